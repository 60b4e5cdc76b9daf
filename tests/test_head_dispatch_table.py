"""The head case table (tests/head_cases.py) against the library's source, on the CPU.

The instantiations of k_head_rows that launch_head can pick are read out of pyz_api.hip: adding one without a case
that reaches it fails here.  The restated kernel choice is pinned at every bucket boundary, and the table is checked
to reach what the GPU matrix promises (both ends of every bucket, each loss branch, activation and edge)."""

import os
import re

import numpy as np
import pytest

from head_cases import CASES, case_data, close_blocks, expected_head_kernel, head_np, head_ut
from oracle import mlp as o_mlp

API = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesian_inference_for_nn_amd", "csrc",
                   "pyz_api.hip")
UTS = (1, 4, 8, 16)
NPS = (4, 8, 12, 16, 24, 32)
K_BUCKET = {1: (1, 64), 4: (65, 256), 8: (257, 512), 16: (513, 1024)}
N_BUCKET = {4: (1, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 24: (17, 24), 32: (25, 32)}


def instantiated_pairs():
    with open(API) as f:
        src = f.read()
    pairs = {(int(u), int(c)) for u, c in re.findall(r"PYZ_HEAD_ROWS_CASE\((\d+),\s*(\d+)\)", src)}
    assert pairs, "no PYZ_HEAD_ROWS_CASE lines found in pyz_api.hip"
    return pairs


def rows_kernel(case):
    """(UT, NP, RW) of a case that runs k_head_rows, else None."""
    m = re.fullmatch(r"k_head_rows<(\d+), (\d+), (\d+)>", case.kernel)
    return tuple(map(int, m.groups())) if m else None


def family(case):
    k = case.kernel
    return "rows" if k.startswith("k_head_rows") else "head" if k == "k_head" else "unfused"


def test_every_instantiation_has_a_case():
    pairs = instantiated_pairs()
    reached = {rk[:2] for c in CASES if (rk := rows_kernel(c)) and rk[2] == 1}
    assert reached == pairs, f"instantiated but no case: {sorted(pairs - reached)}; case but not instantiated: " \
                             f"{sorted(reached - pairs)}"
    # the restated selection rule picks exactly the instantiated pairs
    assert pairs == {(u, c) for u in UTS for c in NPS if u * c <= 128}


def test_every_ut_has_a_four_row_case():
    rw4 = [rk for c in CASES if (rk := rows_kernel(c)) and rk[2] == 4]
    assert {rk[0] for rk in rw4} == set(UTS)
    assert any(rk[1] == 16 for rk in rw4)                                      # DPP softmax
    assert any(rk[1] in (24, 32) and c.loss == "scce" for c in CASES if (rk := rows_kernel(c)) and rk[2] == 4)


def test_rows_cases_sit_at_both_ends_of_each_bucket():
    for ut, np_ in instantiated_pairs():
        cs = [c for c in CASES if (rk := rows_kernel(c)) and rk[:2] == (ut, np_) and rk[2] == 1]
        Ks, Ns = {c.dims[-2] for c in cs}, {c.dims[-1] for c in cs}
        assert set(K_BUCKET[ut]) <= Ks, (ut, np_, sorted(Ks))
        assert set(N_BUCKET[np_]) <= Ns, (ut, np_, sorted(Ns))


@pytest.mark.parametrize("dims, loss, P, batch, kernel", [
    ((8, 64, 4), "scce", 1, 100, "k_head_rows<1, 4, 1>"),
    ((8, 65, 4), "scce", 1, 100, "k_head_rows<4, 4, 1>"),
    ((8, 256, 5), "mse", 1, 100, "k_head_rows<4, 8, 1>"),
    ((8, 257, 8), "mse", 1, 100, "k_head_rows<8, 8, 1>"),
    ((8, 512, 9), "scce", 1, 100, "k_head_rows<8, 12, 1>"),
    ((8, 513, 8), "scce", 1, 100, "k_head_rows<16, 8, 1>"),
    ((8, 1024, 4), "scce", 1, 100, "k_head_rows<16, 4, 1>"),
    ((8, 1025, 4), "scce", 1, 100, "k_head"),
    ((8, 1024, 9), "scce", 1, 100, "k_head"),
    ((8, 512, 16), "scce", 1, 100, "k_head_rows<8, 16, 1>"),
    ((8, 512, 17), "scce", 1, 100, "k_head"),
    ((8, 256, 32), "scce", 1, 100, "k_head_rows<4, 32, 1>"),
    ((8, 256, 33), "scce", 1, 100, "k_loss_scce"),
    ((8, 256, 33), "mse", 1, 100, "k_loss_mse"),
    ((8, 64, 12), "scce", 1, 100, "k_head_rows<1, 12, 1>"),
    ((8, 64, 13), "scce", 1, 100, "k_head_rows<1, 16, 1>"),
    ((8, 64, 17), "scce", 1, 100, "k_head_rows<1, 24, 1>"),
    ((8, 64, 24), "scce", 1, 100, "k_head_rows<1, 24, 1>"),
    ((8, 64, 25), "scce", 1, 100, "k_head_rows<1, 32, 1>"),
    ((784, 200, 10), "scce", 1, 1024, "k_head_rows<4, 12, 1>"),
    ((784, 1024, 10), "scce", 1, 1024, "k_head"),
    ((784, 10), "scce", 1, 1024, "k_head"),
    ((48, 72, 10), "scce", 64, 1003, "k_head_rows<4, 12, 4>"),
    ((48, 72, 10), "scce", 32, 1024, "k_head_rows<4, 12, 4>"),    # P * batch == 32768
    ((48, 72, 10), "scce", 32, 1023, "k_head_rows<4, 12, 1>"),
    ((48, 72, 40), "scce", 64, 1003, "k_loss_scce"),
    ((48, 600, 10), "scce", 64, 1003, "k_head"),
])
def test_expected_head_kernel_at_the_boundaries(dims, loss, P, batch, kernel):
    assert expected_head_kernel(dims, loss, P, batch) == kernel


def test_bucket_helpers():
    assert [head_ut(k) for k in (1, 64, 65, 256, 257, 512, 513, 1024, 1025)] == [1, 1, 4, 4, 8, 8, 16, 16, 0]
    assert [head_np(n) for n in (1, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32)] == [4, 4, 8, 8, 12, 12, 16, 16, 24, 24, 32,
                                                                                   32]


def test_k_head_cases():
    head = [c for c in CASES if family(c) == "head"]
    assert any(256 < c.dims[-2] <= 512 and 17 <= c.dims[-1] <= 32 for c in head)
    assert any(c.dims == (784, 1024, 10) for c in head)
    big_k = [c.dims[-2] for c in head if c.dims[-2] > 1024 and len(c.dims) > 2]
    assert any(k % 8 for k in big_k) and any(k % 8 == 0 for k in big_k)
    l1 = [c for c in head if len(c.dims) == 2]
    assert any(c.gathered for c in l1) and any(not c.gathered for c in l1)
    assert any(c.loss == "mse" for c in head)
    assert {1, 31, 33} <= {c.batch for c in head}
    assert any(c.gathered and c.batch % 32 for c in head)


def test_unfused_boundary_cases():
    assert {(c.dims[-1], c.loss) for c in CASES if family(c) == "unfused"} >= {(33, "scce"), (33, "mse")}


def test_each_mse_activation_in_each_kernel_family():
    for fam in ("rows", "head", "unfused"):
        acts = {c.acts[-1] for c in CASES if family(c) == fam and c.loss == "mse"}
        assert acts >= {"linear", "sigmoid", "tanh", "relu"}, (fam, acts)


def test_each_hidden_activation_in_both_head_kernels():
    for fam in ("rows", "head"):
        acts = {c.acts[-2] for c in CASES if family(c) == fam and len(c.dims) > 2}
        assert acts >= {"relu", "tanh", "sigmoid", "linear"}, (fam, acts)


def test_large_logits_on_every_softmax_path():
    paths = set()
    for c in CASES:
        if c.loss != "scce" or not c.extra.get("logits"):
            continue
        rk = rows_kernel(c)
        paths.add(("dpp" if rk[1] <= 16 else "lane") if rk else c.kernel)
    assert paths >= {"dpp", "lane", "k_head", "k_loss_scce"}, paths


def test_small_edges_are_present():
    assert any(c.extra.get("x_offset") and family(c) == "head" and c.dims[0] % 8 == 0 for c in CASES)
    assert any(c.extra.get("repeat") and c.gathered for c in CASES)
    assert any(c.batch == 1 and family(c) == "rows" for c in CASES)
    assert all(c.batch <= 1003 and c.P <= 64 for c in CASES)


@pytest.mark.parametrize("case", [c for c in CASES if c.extra.get("logits")], ids=lambda c: c.name)
def test_large_logit_data(case):
    """The largest logit of every particle is the requested one (past float32 exp overflow), and with random labels
    the mean loss is of the order of the logits."""
    x, y, idx, thetas = case_data(case)
    rows, ys = (x, y) if idx is None else (x[idx], y[idx])
    for p in range(case.P):
        _, z = o_mlp.forward(thetas[p], rows, case.spec)
        assert abs(z.max() - case.extra["logits"]) < 1e-3 * case.extra["logits"]
        assert z.max() > 88.8
        loss, _, _ = o_mlp.loss_and_grad(thetas[p], rows, ys, case.spec)
        assert loss > 10.0


def test_case_data_is_seeded_and_in_range():
    for c in CASES[:6] + [c for c in CASES if c.gathered][:4]:
        x, y, idx, th = case_data(c)
        x2, y2, idx2, th2 = case_data(c)
        assert np.array_equal(x, x2) and np.array_equal(th, th2) and np.array_equal(y, y2)
        assert th.shape == (c.P, c.spec.n_params) and th.dtype == np.float32
        if c.gathered:
            assert idx.shape == (c.batch,) and idx.min() >= 0 and idx.max() < len(x) and len(x) > c.batch
            if c.extra.get("repeat"):
                assert len(np.unique(idx)) < c.batch
        if c.loss == "scce":
            assert y.min() >= 0 and y.max() < c.dims[-1]


# ---------------------------------------------------------------- close_blocks
SPEC = o_mlp.MLPSpec((200, 50, 10), ("relu", "softmax"), "scce")


def _ref_grad():
    rng = np.random.default_rng(3)
    g = rng.normal(size=SPEC.n_params)
    (_, b0), (k1, b1) = SPEC.offsets()
    g[:b0] *= 10.0           # a large first-layer W block
    g[b1:] *= 1e-3           # a small last-layer bias
    return g


def test_close_blocks_sees_an_error_in_a_small_block():
    ref = _ref_grad()
    (_, _), (_, b1) = SPEC.offsets()
    bad = ref.copy()
    bad[b1 + 3] += 1e-2 * np.abs(ref[b1:]).max()   # 1 % of the last bias: far below 1e-4 of the whole vector
    assert np.abs(bad - ref).max() <= 1e-4 * np.abs(ref).max()
    with pytest.raises(AssertionError, match=r"layer 1 block b"):
        close_blocks(bad, ref, SPEC)
    close_blocks(ref * (1 + 5e-5), ref, SPEC)


def test_close_blocks_floor_and_nonfinite():
    ref = _ref_grad()
    (_, b0), (_, _) = SPEC.offsets()
    ref[b0:b0 + 50] = 0.0                          # a block of exact zeros (dead units)
    g = ref.copy()
    g[b0:b0 + 50] = 1e-8                           # below rel * 1e-3 * max|ref|: passes
    close_blocks(g, ref, SPEC)
    g[b0 + 7] = 1e-3 * np.abs(ref).max()
    with pytest.raises(AssertionError, match=r"layer 0 block b"):
        close_blocks(g, ref, SPEC)
    g = ref.copy()
    g[0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        close_blocks(g, ref, SPEC)
