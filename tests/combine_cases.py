"""The cross-wave combine of the Dense tile kernels (pyz_tile_epilogue, pyz_gemm.h), restated on the host, and forward
inputs whose float32 result depends on the order in which the S wave partials of an output element are added.

The kernels: a workgroup of S waves splits the reduction of one 32 x 32 tile; wave w of k_dense_fwd (scalar path, K not a
multiple of 8) takes the index pairs q = w, w + S, w + 2S, ... (k = 2q, 2q + 1).  Every wave leaves its partial tile in LDS,
and an output element is partial[0] + partial[1] + ... + partial[S - 1], added in float32 one after the other in that order.

The inputs: W holds zeros and ones.  Column n has exactly ONE one inside every wave's index set (at that wave's slot
n % SLOTS), so the partial of wave w for the element (m, n) is exactly one entry of the input row m -- no rounding inside a
wave, whatever its own order.  The input rows hold the terms 2^24, 1, 1, -2^24 (S = 2: 2^24, 1), rotated by m + slot, so
the elements of one output see every rotation.  With these terms the in-order sum, the pairwise tree and the reversed order
give three different float32 results from S = 4 on ((2^24 + 1) + 1) - 2^24 = 0, (2^24 + 1) + (1 - 2^24) = 1,
((-2^24 + 1) + 1) + 2^24 = 2); two terms have one sum in any order, so S = 2 can only show that both partials arrive."""

import numpy as np

import dense_cases as dc

BIG = np.float32(2.0 ** 24)
SLOTS = 14           # index slots per wave that every K below has: u = slot // 2 <= 6, k = 2 (w + S u) + slot % 2 < K
BATCH, N = 70, 40    # the shape whose wave-count boundaries tests/test_dense_dispatch_table.py pins
FIRST_K = {2: 29, 4: 61, 8: 125, 16: 253}    # the first K that gives each S there
# (name, batch, N, K): one case per S, then the column edge and the row edge
FORWARD_CASES = [(f"s{S}", BATCH, N, K) for S, K in FIRST_K.items()] + [("s16_n33", BATCH, 33, 253), ("s16_b33", 33, N, 253)]


def waves_of(batch: int, n: int, k: int) -> int:
    """S of the k_dense_fwd launch (pyz_launch_fwd, restated in dense_cases)."""
    return dc.pick_waves(dc.fwd_tiles(batch, n), dc.fwd_steps(k))[0]


# ---------------------------------------------------------------- the three orders
def combine_in_order(partials: np.ndarray) -> np.ndarray:
    """partials: (S, ...) float32.  Wave 0's partial, then waves 1 .. S - 1 added one after the other, in float32."""
    p = np.asarray(partials, dtype=np.float32)
    s = p[0].copy()
    for w in range(1, p.shape[0]):
        s = (s + p[w]).astype(np.float32)
    return s


def combine_reversed(partials: np.ndarray) -> np.ndarray:
    return combine_in_order(np.asarray(partials, dtype=np.float32)[::-1])


def combine_pairwise(partials: np.ndarray) -> np.ndarray:
    p = [np.asarray(x, dtype=np.float32) for x in partials]
    while len(p) > 1:
        p = [(p[i] + p[i + 1]).astype(np.float32) for i in range(0, len(p), 2)]
    return p[0]


# ---------------------------------------------------------------- the inputs
def terms(S: int) -> np.ndarray:
    base = [BIG, 1.0] if S == 2 else [BIG, 1.0, 1.0, -BIG] * (S // 4)
    return np.asarray(base, dtype=np.float32)


def slot_index(S: int, w: int, slot: int) -> int:
    return 2 * (w + S * (slot // 2)) + slot % 2


def wave_of_index(S: int, k: int) -> int:
    return (k >> 1) % S


def forward_inputs(batch: int, n: int, k: int, S: int):
    """(A (batch, k), W (k, n), bias (n)) as float32."""
    t = terms(S)
    a = np.zeros((batch, k), np.float32)
    w = np.zeros((k, n), np.float32)
    for wave in range(S):
        for slot in range(SLOTS):
            kk = slot_index(S, wave, slot)
            assert kk < k and wave_of_index(S, kk) == wave
            for m in range(batch):
                a[m, kk] = t[(wave + m + slot) % S]
        for col in range(n):
            w[slot_index(S, wave, col % SLOTS), col] = 1.0
    return a, w, np.zeros((n,), np.float32)


def wave_partials(a: np.ndarray, w: np.ndarray, bias: np.ndarray, S: int) -> np.ndarray:
    """(S, batch, n): every wave's partial tile.  Exact for the inputs above (one non-zero product per wave and element),
    which is asserted; the bias rides in wave 0."""
    batch, k = a.shape
    n = w.shape[1]
    out = np.zeros((S, batch, n), np.float64)
    for wave in range(S):
        ks = [kk for kk in range(k) if wave_of_index(S, kk) == wave]
        prod = a[:, ks, None].astype(np.float64) * w[None, ks, :].astype(np.float64)
        assert np.all((prod != 0).sum(axis=1) <= 1), "more than one term inside a wave: its partial would depend on its own order"
        out[wave] = prod.sum(axis=1)
    out[0] += bias.astype(np.float64)
    assert np.array_equal(out, out.astype(np.float32).astype(np.float64))
    return out.astype(np.float32)


def host_forward(a, w, bias, S, combine=combine_in_order) -> np.ndarray:
    return combine(wave_partials(a, w, bias, S))
