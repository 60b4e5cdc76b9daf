"""The order of the cross-wave combine (pyz_tile_epilogue), on the CPU: the host restatement that the GPU test compares
with (tests/combine_cases.py) adds the wave partials 0 .. S - 1 one after the other in float32, and on the inputs of that
test this order is told apart from a pairwise tree and from the reversed order."""

import numpy as np
import pytest

import combine_cases as cc


def test_the_three_orders_on_four_terms():
    p = np.asarray([cc.BIG, 1.0, 1.0, -cc.BIG], np.float32).reshape(4, 1)
    assert cc.combine_in_order(p)[0] == 0.0      # ((2^24 + 1) + 1) - 2^24: both ones are lost
    assert cc.combine_pairwise(p)[0] == 1.0      # (2^24 + 1) + (1 - 2^24): one survives
    assert cc.combine_reversed(p)[0] == 2.0      # ((-2^24 + 1) + 1) + 2^24: both survive
    assert cc.combine_in_order(p).dtype == np.float32


def test_in_order_is_a_float32_chain_from_wave_zero():
    rng = np.random.default_rng(3)
    p = (rng.standard_normal((16, 5, 7)) * 10.0 ** rng.integers(-3, 4, (16, 5, 7))).astype(np.float32)
    want = p[0].copy()
    for w in range(1, 16):
        want = want + p[w]                          # float32 + float32 stays float32
    assert want.dtype == np.float32
    assert np.array_equal(cc.combine_in_order(p).view(np.int32), want.view(np.int32))
    wide = p.astype(np.float64).sum(axis=0).astype(np.float32)          # a float64 accumulation is another function
    assert not np.array_equal(cc.combine_in_order(p).view(np.int32), wide.view(np.int32))


@pytest.mark.parametrize("name,batch,n,k", cc.FORWARD_CASES, ids=[c[0] for c in cc.FORWARD_CASES])
def test_inputs_tell_the_orders_apart(name, batch, n, k):
    S = cc.waves_of(batch, n, k)
    assert S == int(name.split("_")[0][1:])
    a, w, bias = cc.forward_inputs(batch, n, k, S)
    assert set(np.unique(w)) == {0.0, 1.0} and np.all(w.sum(axis=0) == S)     # one selected index per wave and column
    parts = cc.wave_partials(a, w, bias, S)
    assert np.all(parts != 0)                                                  # every wave contributes to every element
    want = cc.host_forward(a, w, bias, S)
    # a float64 sum of the terms is 2 S / 4 (S = 2: 2^24 + 1): the float32 chain loses ones on the way, by its order
    exact = parts.astype(np.float64).sum(axis=0)
    assert np.all(exact == (float(cc.BIG) + 1.0 if S == 2 else S / 2))
    pair, rev = cc.host_forward(a, w, bias, S, cc.combine_pairwise), cc.host_forward(a, w, bias, S, cc.combine_reversed)
    if S == 2:
        # two terms: every order is the same sum; the case shows that both waves' partials arrive (one alone gives 1 or 2^24)
        assert np.array_equal(pair, want) and np.array_equal(rev, want) and np.all(want == cc.BIG)
        return
    for other, what in ((pair, "pairwise tree"), (rev, "reversed")):
        differs = other != want
        assert differs.mean() >= 0.25, f"{what}: only {differs.mean():.2f} of the elements differ from the in-order sum"
        assert differs.any(axis=1).all() and differs.any(axis=0).all(), f"{what}: a row or a column cannot tell"


def test_first_k_of_every_wave_count():
    """The K of the cases are the boundaries tests/test_dense_dispatch_table.py pins (batch 70, N = 40)."""
    for S, k in cc.FIRST_K.items():
        assert cc.waves_of(cc.BATCH, cc.N, k) == S and cc.waves_of(cc.BATCH, cc.N, k - 1) == S // 2
        assert k % 8 != 0                                  # the scalar path: wave w owns the index pairs w, w + S, ...
        assert cc.slot_index(S, S - 1, cc.SLOTS - 1) < k
