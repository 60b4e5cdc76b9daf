"""The loss-head case table and its shared checks (a plain module: imported by the head tests, not a conftest).

Every gradient step ends in the head: the last Dense layer, the loss, delta_L and delta_{L-1} in one kernel.
Which kernel runs is decided from the model's shape alone; `expected_head_kernel` restates that choice and `CASES`
lists shapes that, together, reach every instantiation of it, with the edges where such kernels go wrong."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import mlp as o_mlp

RW_ROWS = 32768   # default of PYZ_HEAD_RW_ROWS: P * batch at or above it gives every head wave four rows


def head_ut(K: int) -> int:
    """Hidden units per lane of k_head_rows for a last layer of K inputs (0: too wide for it)."""
    return 1 if K <= 64 else 4 if K <= 256 else 8 if K <= 512 else 16 if K <= 1024 else 0


def head_np(N: int) -> int:
    """Class count padded for k_head_rows."""
    return next(c for c in (4, 8, 12, 16, 24, 32) if N <= c)


def expected_head_kernel(dims, loss: str, P: int, batch: int) -> str:
    """The kernel `MLPPlan.loss_grad` runs for the loss (the name KernelProbe reports).

    Restates csrc/pyz_api.hip: can_fuse and launch_loss_backward (a last layer wider than 32 goes to the unfused
    launch_loss: k_loss_scce / k_loss_mse), then launch_head (UT from K = dims[L-1], NP from N = dims[L]; k_head_rows
    when UT * NP <= 128 with RW from the PYZ_HEAD_RW_ROWS default, else k_head)."""
    K, N = dims[-2], dims[-1]
    if N > 32:
        return "k_loss_scce" if loss == "scce" else "k_loss_mse"
    UT, NP = head_ut(K), head_np(N)
    if UT and UT * NP <= 128:
        RW = 4 if P * batch >= RW_ROWS else 1
        return f"k_head_rows<{UT}, {NP}, {RW}>"
    return "k_head"


class HeadCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str
    P: int = 1
    batch: int = 64
    gathered: bool = False   # x has more rows than the batch; the batch comes through row_idx
    extra: dict = {}         # logits: scale the last layer so the largest logit is this; x_offset: x starts 4 bytes
    #                          into its storage; repeat: row_idx repeats rows

    @property
    def spec(self) -> o_mlp.MLPSpec:
        return o_mlp.MLPSpec(self.dims, self.acts, self.loss)

    @property
    def kernel(self) -> str:
        return expected_head_kernel(self.dims, self.loss, self.P, self.batch)


def _c(name, dims, acts, loss, P=1, batch=64, gathered=False, **extra):
    return HeadCase(name, tuple(dims), tuple(acts), loss, P, batch, gathered, extra)


S, M = "scce", "mse"
BIG = {"logits": 150.0}   # past float32 exp overflow (~88.7): a softmax without max subtraction gives inf / nan

CASES = [
    # ---- k_head_rows, one row per wave: every (UT, NP) pair with K and N at both ends of their buckets
    _c("rows_1x4_lo", (9, 1, 1), ("tanh", "linear"), M, batch=37),
    _c("rows_1x4_hi", (16, 64, 4), ("relu", "softmax"), S, P=2, batch=50, gathered=True),
    _c("rows_1x8_lo_batch1", (7, 1, 5), ("sigmoid", "softmax"), S, batch=1),
    _c("rows_1x8_hi", (12, 64, 8), ("linear", "sigmoid"), M),
    _c("rows_1x12_lo_dpp_big", (1, 9), ("softmax",), S, batch=70, gathered=True, **BIG),
    _c("rows_1x12_hi_repeat", (8, 64, 12), ("tanh", "tanh"), M, P=2, batch=45, gathered=True, repeat=True),
    _c("rows_1x16_lo", (12, 1, 13), ("sigmoid", "relu"), M, batch=40),
    _c("rows_1x16_hi", (16, 64, 16), ("relu", "softmax"), S, P=3, batch=120, gathered=True),
    _c("rows_1x24_lo_lane_big", (1, 17), ("softmax",), S, batch=90, **BIG),
    _c("rows_1x24_hi", (16, 64, 24), ("linear", "linear"), M, batch=33),
    _c("rows_1x32_lo", (5, 1, 25), ("relu", "sigmoid"), M, P=2, batch=77, gathered=True),
    _c("rows_1x32_hi", (12, 64, 32), ("sigmoid", "softmax"), S, batch=100),
    _c("rows_4x4_lo", (12, 65, 1), ("relu", "linear"), M),
    _c("rows_4x4_hi", (16, 256, 4), ("tanh", "softmax"), S, batch=80),
    _c("rows_4x8_lo", (20, 65, 5), ("linear", "softmax"), S, P=2, batch=60, gathered=True),
    _c("rows_4x8_hi", (8, 256, 8), ("sigmoid", "tanh"), M, batch=50),
    _c("rows_4x12_lo", (16, 65, 9), ("relu", "linear"), M, batch=41),
    _c("rows_4x12_hi_xoff", (16, 256, 12), ("tanh", "softmax"), S, batch=96, x_offset=True),
    _c("rows_4x16_lo", (12, 65, 13), ("sigmoid", "softmax"), S, batch=57),
    _c("rows_4x16_hi", (16, 256, 16), ("relu", "sigmoid"), M, batch=64),
    _c("rows_4x24_lo", (10, 65, 17), ("relu", "relu"), M, batch=48),
    _c("rows_4x24_hi", (16, 256, 24), ("tanh", "softmax"), S, P=2, batch=72, gathered=True),
    _c("rows_4x32_lo_lane_big", (12, 65, 25), ("sigmoid", "softmax"), S, batch=66, **BIG),
    _c("rows_4x32_hi", (16, 256, 32), ("linear", "tanh"), M, batch=35),
    _c("rows_8x4_lo", (12, 257, 1), ("tanh", "linear"), M, batch=52),
    _c("rows_8x4_hi", (16, 512, 4), ("relu", "softmax"), S, batch=64),
    _c("rows_8x8_lo", (12, 257, 5), ("sigmoid", "sigmoid"), M, batch=39),
    _c("rows_8x8_hi", (16, 512, 8), ("linear", "softmax"), S, batch=70),
    _c("rows_8x12_lo", (12, 257, 9), ("relu", "softmax"), S, batch=45, gathered=True),
    _c("rows_8x12_hi", (16, 512, 12), ("tanh", "relu"), M, batch=64),
    _c("rows_8x16_lo", (12, 257, 13), ("sigmoid", "tanh"), M, batch=38),
    _c("rows_8x16_hi", (16, 512, 16), ("relu", "softmax"), S, P=2, batch=90, gathered=True),
    _c("rows_16x4_lo", (12, 513, 1), ("relu", "sigmoid"), M, batch=47),
    _c("rows_16x4_hi", (16, 1024, 4), ("tanh", "softmax"), S, batch=64, gathered=True),
    _c("rows_16x8_lo", (12, 513, 5), ("sigmoid", "softmax"), S, batch=61),
    _c("rows_16x8_hi", (16, 1024, 8), ("linear", "relu"), M, batch=36),
    # ---- k_head_rows, other shapes: one layer (the data rows are the head's input, gathered or not), three layers,
    # a common classifier that runs the per-lane softmax
    _c("rows_l1_gathered", (20, 6), ("softmax",), S, P=2, batch=83, gathered=True),
    _c("rows_l1_mse", (64, 3), ("linear",), M, batch=58),
    _c("rows_l3", (12, 40, 200, 10), ("relu", "tanh", "softmax"), S, batch=75),
    _c("rows_784_256_20", (784, 256, 20), ("relu", "softmax"), S, batch=128, gathered=True),
    # ---- k_head_rows, four rows per wave (64 particles x 1003 gathered rows): every UT, DPP and per-lane softmax
    _c("rw4_1x32_lane", (12, 50, 30), ("relu", "softmax"), S, P=64, batch=1003, gathered=True),
    _c("rw4_4x16_dpp", (12, 200, 16), ("tanh", "softmax"), S, P=64, batch=1003, gathered=True),
    _c("rw4_4x24_mse", (12, 130, 20), ("sigmoid", "tanh"), M, P=64, batch=1003, gathered=True),
    _c("rw4_8x12", (12, 300, 10), ("relu", "softmax"), S, P=64, batch=1003, gathered=True),
    _c("rw4_16x8", (12, 1024, 8), ("relu", "softmax"), S, P=64, batch=1003, gathered=True),
    # ---- k_head (MFMA): last layers too large for lane-resident operands
    _c("head_k300_n20", (16, 300, 20), ("relu", "softmax"), S, P=2, batch=96),
    _c("head_k512_n32_mse_sigmoid", (12, 512, 32), ("tanh", "sigmoid"), M, batch=70),
    _c("head_784_1024_10", (784, 1024, 10), ("relu", "softmax"), S, batch=128, gathered=True),
    _c("head_k1100_vec0", (12, 1100, 10), ("sigmoid", "softmax"), S, batch=70),
    _c("head_k1152_vec1", (16, 1152, 6), ("linear", "softmax"), S, batch=64),
    _c("head_l1", (784, 10), ("softmax",), S, batch=64),
    _c("head_l1_gathered", (784, 10), ("softmax",), S, P=2, batch=203, gathered=True),
    _c("head_l1_xoff", (784, 10), ("softmax",), S, batch=77, x_offset=True),
    _c("head_mse_linear", (12, 600, 24), ("relu", "linear"), M, batch=66),
    _c("head_mse_tanh", (12, 520, 12), ("sigmoid", "tanh"), M, batch=45),
    _c("head_mse_relu", (16, 1030, 3), ("tanh", "relu"), M, batch=50),
    _c("head_big", (16, 700, 16), ("relu", "softmax"), S, batch=80, **BIG),
    _c("head_batch1", (12, 600, 12), ("tanh", "softmax"), S, batch=1),
    _c("head_batch31", (12, 600, 12), ("tanh", "softmax"), S, batch=31),
    _c("head_batch33", (12, 600, 12), ("tanh", "softmax"), S, batch=33),
    _c("head_ragged_gathered", (12, 640, 10), ("relu", "softmax"), S, batch=1003, gathered=True, repeat=True),
    # ---- unfused loss kernels: last layers wider than one 32-column tile
    _c("unf_scce_33", (12, 40, 33), ("relu", "softmax"), S, batch=70),
    _c("unf_scce_big", (12, 50, 40), ("relu", "softmax"), S, batch=60, **BIG),
    _c("unf_mse_33_linear", (12, 40, 33), ("tanh", "linear"), M, batch=55, gathered=True),
    _c("unf_mse_sigmoid", (12, 30, 40), ("relu", "sigmoid"), M, batch=44),
    _c("unf_mse_tanh", (10, 20, 36), ("sigmoid", "tanh"), M, batch=39),
    _c("unf_mse_relu", (8, 24, 48), ("linear", "relu"), M, batch=42),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"


def case_data(case: HeadCase):
    """Seeded inputs of a case: (x rows, labels / targets, row_idx or None, thetas (P, D)), all float32 / int32.
    Weights are scaled by fan-in so every layer's pre-activations are O(1); a `logits` case then scales each particle's
    last layer so its largest logit over the batch is exactly that value."""
    spec = case.spec
    rng = np.random.default_rng(sum(map(ord, case.name)))
    n_rows = case.batch + case.batch // 5 + 3 if case.gathered else case.batch
    x = rng.normal(size=(n_rows, spec.dims[0])).astype(np.float32)
    N = spec.dims[-1]
    if case.loss == "scce":
        y = rng.integers(0, N, size=n_rows).astype(np.int32)
    elif spec.acts[-1] == "sigmoid":
        y = rng.uniform(0.0, 1.0, size=(n_rows, N)).astype(np.float32)
    elif spec.acts[-1] == "tanh":
        y = rng.uniform(-1.0, 1.0, size=(n_rows, N)).astype(np.float32)
    else:
        y = rng.normal(size=(n_rows, N)).astype(np.float32)
    idx = None
    if case.gathered:
        idx = rng.permutation(n_rows)[:case.batch].astype(np.int32)
        if case.extra.get("repeat"):
            idx = rng.integers(0, n_rows, size=case.batch).astype(np.int32)   # repeats by chance ...
            idx[1::7] = idx[0]                                                # ... and one row many times
    thetas = np.empty((case.P, spec.n_params), dtype=np.float32)
    for p in range(case.P):
        parts = []
        for fan_in, fan_out in zip(spec.dims[:-1], spec.dims[1:]):
            parts.append(rng.normal(size=fan_in * fan_out) * (1.5 / np.sqrt(fan_in)))
            parts.append(rng.normal(size=fan_out) * 0.2)
        thetas[p] = np.concatenate(parts).astype(np.float32)
    big = case.extra.get("logits")
    if big:
        ko, _ = spec.offsets()[-1]
        rows = x if idx is None else x[idx]
        for p in range(case.P):
            _, z = o_mlp.forward(thetas[p], rows, spec)
            thetas[p, ko:] = (thetas[p, ko:].astype(np.float64) * (big / z.max())).astype(np.float32)
    return x, y, idx, thetas


def check_particles(P: int):
    """The particles a case compares with the oracle: the first, the middle and the last."""
    return sorted({0, P // 2, P - 1})


def close_blocks(grad, ref, spec: o_mlp.MLPSpec, rel: float = 1e-4, what: str = "grad", state=None) -> float:
    """Each layer's W and b block against the reference on its own scale:
    max|g - r| <= rel * max(max|r_block|, 1e-3 * max|r|).  The floor only keeps a block of exact zeros (dead units)
    from demanding bit equality.  `state` (for a difference of two stored float32 vectors: the vector of their larger
    magnitudes) adds 2^-23 * max|state_block| to a block's tolerance: the two float32 roundings of what was stored.
    Returns the largest error over tolerance of any block."""
    grad = np.asarray(grad.detach().cpu().numpy() if hasattr(grad, "detach") else grad, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert grad.shape == ref.shape, (what, grad.shape, ref.shape)
    assert np.all(np.isfinite(grad)), f"{what}: non-finite gradient entries"
    floor = 1e-3 * np.abs(ref).max()
    worst = 0.0
    for l, ((ko, bo), K, N) in enumerate(zip(spec.offsets(), spec.dims[:-1], spec.dims[1:])):
        for block, lo, shape in (("W", ko, (K, N)), ("b", bo, (N,))):
            g = grad[lo:lo + int(np.prod(shape))]
            r = ref[lo:lo + int(np.prod(shape))]
            scale = max(np.abs(r).max(), floor)
            tol = rel * scale
            if state is not None:
                tol += 2.0 ** -23 * float(np.abs(np.asarray(state, dtype=np.float64).reshape(-1)[lo:lo + int(np.prod(shape))]).max())
            diff = np.abs(g - r)
            err = diff.max()
            if not err <= tol:
                i = int(diff.argmax())
                at = tuple(map(int, np.unravel_index(i, shape)))
                raise AssertionError(f"{what}: layer {l} block {block} {shape}: max err {err:.3e} at {at} "
                                     f"(gpu {g[i]:.6e}, ref {r[i]:.6e}) vs block scale {scale:.3e}, tolerance {tol:.3e} "
                                     f"(rel {err / max(scale, 1e-300):.3e} > {rel:g})")
            worst = max(worst, err / tol if tol > 0 else 0.0)
    return worst
