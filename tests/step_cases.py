"""The case table of the eager SGD, SWAG, SGLD and BBB steps and the comparison both step tests share (a plain module).

An eager step runs its update either in the epilogue of k_wgrad_all<S> (a last layer of at most 32 units: `pyz_update_math`,
`pyz_update_store`, the per-mode prefetch) or in a kernel of its own behind the per-layer weight gradients (k_sgd_update,
k_swag_update, k_sgld_update, k_bbb_sample with k_bbb_update).  This module restates which of them a (case, mode) launches
(`expected_step_launches`, on top of dense_cases.expected_launches), names the cells of the coverage table (`CELLS`,
`reached_cells`), lists cases that reach every cell with every mode, builds their data (dense_cases.case_data plus a
non-zero starting state), restates one step of each mode on top of oracle.mlp in a chosen dtype, with the wrong variants
the sensitivity check needs (`ref_step`, `MUTATIONS`), and holds the comparison of one step (`compare_step`).
tests/test_step_dispatch_table.py pins all of it to the source and to the oracle modules on the CPU;
tests/test_gpu_step_matrix.py runs the cases on the device."""

from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from dense_cases import DenseCase, batch_rows, can_fuse, case_data, expected_launches
from head_cases import close_blocks
from oracle import mlp as o_mlp
from oracle import philox as o_philox

# ---------------------------------------------------------------- the rules (csrc/pyz_fused.h, pyz_api.hip)
MODES = ("sgd", "swag", "sgld", "bbb")
UPD_MODE = {"none": 0, "sgd": 1, "sgld": 2, "bbb": 3, "swag": 4}     # PYZ_UPD_*
UPDATE_KERNEL = {"sgd": "k_sgd_update", "swag": "k_swag_update", "sgld": "k_sgld_update", "bbb": "k_bbb_update"}
SAMPLE_KERNEL = "k_bbb_sample"             # pyz_bbb_step launches it first on either path
PER_THREAD = {"k_sgd_update": 1, "k_swag_update": 1, "k_sgld_update": 4, "k_bbb_sample": 4, "k_bbb_update": 4}
STREAM = {"sgld": 0, "bbb": 1}             # PYZ_STREAM_SGLD, PYZ_STREAM_BBB
VARIANTS = {"sgd": ("plain",), "swag": ("plain",), "sgld": ("zeros", "philox", "device"), "bbb": ("philox", "device")}
N_STEPS = 3
# the three SWAG steps of a case: (update_moments, deviation row passed: index into the two rows, or None)
SWAG_STEPS = ((True, 1), (False, 0), (True, None))
SS = (1, 2, 4, 8, 16)
BLOCK = 1024                               # elements of one 256-thread block of the 4-per-thread kernels


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def update_grid(kernel: str, D: int) -> int:
    """Blocks of 256 threads: cdiv(D, 256) for the one-element kernels, cdiv(cdiv(D, 4), 256) for the others."""
    return cdiv(cdiv(D, PER_THREAD[kernel]), 256)


class StepCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str
    batch: int
    gathered: bool = False
    lr: float = 0.5          # SGD / SWAG / SGLD: every block's lr max|g| is at least 0.5 % of max|theta0|
    bbb_lr: float = 0.5      # BBB: small enough that rho stays where float32 keeps the data gradient through three steps
    n0: int = 3              # step count of the first of the three steps
    alpha: float = 0.0625    # BBB: weight of log q - log p
    prior: tuple = (0.125, 0.75)   # BBB: scalar prior mean and raw rho
    seed: int = 11           # Philox seed
    prior_vec: bool = False  # BBB: per-element prior vectors (the scalars are passed too and must be ignored)
    aligned: bool = False    # state buffers 16-byte aligned (else 4 bytes off)
    data_seed: int = 0

    @property
    def spec(self) -> o_mlp.MLPSpec:
        return o_mlp.MLPSpec(self.dims, self.acts, self.loss)

    @property
    def D(self) -> int:
        return self.spec.n_params

    @property
    def fused(self) -> bool:
        return can_fuse(self.dims)

    @property
    def dense(self) -> DenseCase:
        """The Dense case with this shape whose gradient call carries an update (dense_cases: sgd=True)."""
        return DenseCase(self.name, self.dims, self.acts, self.loss, 1, self.batch, self.gathered, False, {}, self.fused,
                         self.data_seed)

    @property
    def max_batch(self) -> int:
        return self.batch + 3


class StepLaunches(NamedTuple):
    sample: int        # k_bbb_sample launches
    wgrad: tuple       # kernel expressions KernelProbe reports, in launch order
    update: tuple      # the mode's own update kernel (unfused) or nothing
    S: int             # waves of k_wgrad_all (0 when unfused)
    gather: str        # "none", "copy" or "self"


def expected_step_launches(case: StepCase, mode: str) -> StepLaunches:
    """pyz_sgd_step / pyz_swag_step / launch_sgld_step / pyz_bbb_step: fused = one k_wgrad_all<S> with the mode's update in
    its epilogue; else k_dense_bwd_weight per layer (mode PYZ_UPD_NONE into m->grad) and then the mode's update kernel."""
    la = expected_launches(case.dense)
    wg = tuple(w.kernel for w in la.wgrad)
    gathers = {w.gather for w in la.wgrad} - {""}
    assert len(gathers) <= 1
    gather = gathers.pop() if gathers else "none"
    if case.fused:
        assert len(wg) == 1 and "true" not in wg[0]
        return StepLaunches(int(mode == "bbb"), wg, (), la.wgrad[0].S, gather)
    assert wg == ("k_dense_bwd_weight",) * (len(case.dims) - 1)
    return StepLaunches(int(mode == "bbb"), wg, (UPDATE_KERNEL[mode],), 0, gather)


# ---------------------------------------------------------------- the coverage table
UNFUSED_GROUPS = {"sgd": "k_sgd_update", "swag": "k_swag_update", "sgld": "k_sgld_update", "bbb": "k_bbb_sample+k_bbb_update"}
CELLS = frozenset(
    [f"{m} S={S}" for m in MODES for S in SS] +
    [f"{m} gather={g}" for m in MODES for g in ("none", "copy", "self")] +
    [f"{k} D%4={r}" for k in UNFUSED_GROUPS.values() for r in range(4)] +
    ["unfused D spans more than one 1024-element block", "state buffers 4 bytes off 16-byte alignment",
     "state buffers 16-byte aligned", "SWAG step without update", "SWAG dev_row None on an update step",
     "BBB per-element prior vectors", "odd batch", "K + 1 = 32", "K + 1 = 33", "ragged N"])


def reached_cells(case: StepCase, modes=MODES) -> set:
    """The cells a case reaches with the given modes, from its shape and `expected_step_launches` alone."""
    cells = set()
    for m in modes:
        la = expected_step_launches(case, m)
        cells.add(f"{m} gather={la.gather}")
        if case.fused:
            cells.add(f"{m} S={la.S}")
        else:
            cells.add(f"{UNFUSED_GROUPS[m]} D%4={case.D % 4}")
            if case.D > BLOCK:
                cells.add("unfused D spans more than one 1024-element block")
        if m == "swag":
            cells |= {"SWAG step without update", "SWAG dev_row None on an update step"}
        if m == "bbb" and case.prior_vec:
            cells.add("BBB per-element prior vectors")
    cells.add("state buffers 16-byte aligned" if case.aligned else "state buffers 4 bytes off 16-byte alignment")
    if case.batch % 2:
        cells.add("odd batch")
    for K, N in zip(case.dims[:-1], case.dims[1:]):
        if K + 1 in (32, 33):
            cells.add(f"K + 1 = {K + 1}")
        if N % 32:
            cells.add("ragged N")
    return cells & CELLS


R, T, G, LN, SM = "relu", "tanh", "sigmoid", "linear", "softmax"
SC, MS = "scce", "mse"


def _c(name, dims, acts, loss, batch, **kw):
    return StepCase(name, tuple(dims), tuple(acts), loss, batch, **kw)


CASES = [
    # ---- fused: the update in the epilogue of k_wgrad_all<S>, every S, every gather, odd / even batches
    _c("f_s1", (20, 16, 4), (R, SM), SC, 14),
    _c("f_s1_aligned", (20, 16, 4), (R, SM), SC, 15, aligned=True, prior_vec=True, bbb_lr=0.25),
    _c("f_s2_odd", (31, 20, 10), (T, SM), SC, 33, prior_vec=True),
    _c("f_s4_copy", (32, 24, 10), (T, SM), SC, 64, gathered=True),
    _c("f_s4_self_l1", (31, 10), (SM,), SC, 63, gathered=True),
    _c("f_s8_l3", (16, 31, 32, 10), (R, R, SM), SC, 128, bbb_lr=0.25),
    _c("f_s16_l3_mse", (20, 32, 31, 6), (G, T, LN), MS, 301, gathered=True, prior_vec=True, bbb_lr=0.25),
    # ---- unfused (last layer wider than 32): k_dense_bwd_weight per layer, then the mode's own update kernel; D % 4 of
    # 0 .. 3, one and several 1024-element blocks
    _c("u_d99", (2, 33), (SM,), SC, 9, bbb_lr=0.125),
    _c("u_d165_mse", (4, 33), (LN,), MS, 16, prior_vec=True, bbb_lr=0.0625),
    _c("u_d218_self", (3, 5, 33), (T, SM), SC, 31, gathered=True),
    _c("u_d1100", (12, 20, 40), (T, SM), SC, 70, data_seed=2),
    _c("u_d1100_aligned", (12, 20, 40), (T, SM), SC, 70, aligned=True, data_seed=1),
    _c("u_d2596_mse", (30, 36, 40), (R, LN), MS, 45, bbb_lr=0.03125),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"


# ---------------------------------------------------------------- data
class StepData(NamedTuple):
    x: np.ndarray
    y: np.ndarray
    idx: Optional[np.ndarray]
    rows: np.ndarray         # the batch rows and their targets
    ys: np.ndarray
    theta0: np.ndarray       # float32 (D): theta of SGD / SWAG / SGLD, mu of BBB
    mean0: np.ndarray        # near theta0
    sq0: np.ndarray          # >= mean0^2
    dev0: np.ndarray         # (2, D): the deviation rows before the first step
    rho0: np.ndarray         # uniform in [-3, 1]
    pm_vec: Optional[np.ndarray]
    pr_vec: Optional[np.ndarray]


def step_data(case: StepCase) -> StepData:
    """dense_cases.case_data (edges weighted) and a starting state that is not zero: the moments as if earlier steps had
    passed (mean0 within a tenth of theta's rms of theta0, sq0 = mean0^2 + a positive variance), two deviation rows of
    arbitrary values, rho0 uniform in [-3, 1] (sigma 0.05 .. 1.3: below that float32 itself loses the data gradient in
    d mu + d w, where alpha d / sigma^2 cancels), per-element priors around the scalar ones."""
    x, y, idx, thetas = case_data(case.dense)
    rows, ys = batch_rows(case.dense, x, y, idx)
    theta0 = thetas[0]
    D = theta0.size
    rng = np.random.default_rng(sum(map(ord, case.name)) + 7919 * (case.data_seed + 1))
    rms = float(np.sqrt(np.mean(theta0.astype(np.float64) ** 2)))
    mean0 = (theta0 + 0.1 * rms * rng.normal(size=D)).astype(np.float32)
    sq0 = (mean0.astype(np.float64) ** 2 + (0.05 * rms * (1.0 + rng.uniform(size=D))) ** 2).astype(np.float32)
    dev0 = rng.normal(size=(2, D)).astype(np.float32)
    rho0 = rng.uniform(-3.0, 1.0, size=D).astype(np.float32)
    pm_vec = pr_vec = None
    if case.prior_vec:
        pm_vec = rng.uniform(-0.5, 0.5, size=D).astype(np.float32)
        pr_vec = rng.uniform(0.25, 1.5, size=D).astype(np.float32)
    return StepData(x, y, idx, rows, ys, theta0, mean0, sq0, dev0, rho0, pm_vec, pr_vec)


def initial_state(mode: str, data: StepData) -> dict:
    if mode == "sgd":
        return {"theta": data.theta0.copy()}
    if mode == "sgld":
        return {"theta": data.theta0.copy(), "mean": data.mean0.copy(), "sq": data.sq0.copy()}
    if mode == "swag":
        return {"theta": data.theta0.copy(), "mean": data.mean0.copy(), "sq": data.sq0.copy(), "dev": data.dev0.copy()}
    return {"mu": data.theta0.copy(), "rho": data.rho0.copy(), "w": np.zeros_like(data.theta0)}


def injected_noise(case: StepCase, mode: str, variant: str, k: int):
    """The float32 vector a step is given as unit_noise / eps (None: the device draws it)."""
    if variant == "zeros":
        return np.zeros(case.D, dtype=np.float32)
    if variant == "philox":
        return o_philox.normal(case.seed, STREAM[mode], case.n0 + k, case.D).astype(np.float32)
    return None


# ---------------------------------------------------------------- one step, restated on oracle.mlp (any dtype, wrong variants)
MUTATIONS = {   # name -> the modes it applies to
    "noise drawn for element e + 1": ("sgld", "bbb"),
    "noise of the last 4-group zero": ("sgld", "bbb"),
    "noise scaled by lr instead of lr^2": ("sgld",),
    "last layer's bias gradient scaled by 1.001": MODES,
    "last row of W0's gradient dropped": MODES,
    "moments with count n + 1": ("sgld", "swag"),
    "deviation against the old mean": ("swag",),
    "moments written on a non-update step": ("swag",),
    "BBB d rho with the wrong sign": ("bbb",),
    "BBB prior vector ignored": ("bbb",),
    "BBB rho update without eps": ("bbb",),
    "log q - log p without the prior term": ("bbb",),
}
_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)   # a Python float: keeps float32 arithmetic in float32


def mutation_applies(case: StepCase, mode: str, variant: str, mutation: str) -> bool:
    if mode not in MUTATIONS[mutation]:
        return False
    if mutation.startswith("noise"):
        return variant != "zeros"
    if mutation == "BBB prior vector ignored":
        return case.prior_vec
    if mode == "sgld" and "gradient" in mutation:
        return variant == "zeros"     # beside the Langevin noise the gradient term is not on its own scale
    return True


def _gradient(theta, data: StepData, spec, dt, mutation):
    loss, g, _ = o_mlp.loss_and_grad(theta, data.rows, data.ys, spec, dt)
    if mutation == "last layer's bias gradient scaled by 1.001":
        bo = spec.offsets()[-1][1]
        g[bo:] = g[bo:] * dt(1.001)
    if mutation == "last row of W0's gradient dropped":
        K, N = spec.dims[0], spec.dims[1]
        g[(K - 1) * N:K * N] = 0
    return loss, g


def _noise(case: StepCase, mode: str, variant: str, k: int, dt, mutation):
    """The N(0, 1) vector of a step as the arithmetic sees it: the injected float32 values, or (device) the float64 draws."""
    D, n = case.D, case.n0 + k
    if variant == "zeros":
        return np.zeros(D, dtype=dt)
    z = o_philox.normal(case.seed, STREAM[mode], n, D + 1)
    z = z[1:] if mutation == "noise drawn for element e + 1" else z[:D]
    if variant == "philox":
        z = z.astype(np.float32)
    z = z.astype(dt)
    if mutation == "noise of the last 4-group zero":
        z[4 * ((D - 1) // 4):] = 0
    return z


def _softplus(x):
    return np.logaddexp(0.0, x)


def ref_step(case: StepCase, data: StepData, mode: str, variant: str, k: int, s0: dict, dtype=np.float64, mutation=None) -> dict:
    """Step k (count n = n0 + k) of `mode` from the state s0, in `dtype`: the arithmetic of oracle.sgd / swag / sgld / bbb
    (tests/test_step_dispatch_table.py holds the two equal, bit for bit, in float64 and float32), with `mutation` one of
    the wrong variants above.  Returns the new state and the loss (BBB: cost = [cost, data loss, log q - log p] and
    kl_abs = sum_e |log q_e| + |log p_e|)."""
    dt, spec = dtype, case.spec
    lr, n = dt(case.lr), dt(case.n0 + k)
    if mode == "bbb":
        return _ref_bbb(case, data, variant, k, s0, dt, mutation)
    theta0 = np.asarray(s0["theta"], dtype=dt)
    loss, g = _gradient(theta0, data, spec, dt, mutation)
    out = {"loss": loss}
    if mode == "sgd":
        out["theta"] = theta0 - lr * g
        return out
    mean0, sq0 = np.asarray(s0["mean"], dtype=dt), np.asarray(s0["sq"], dtype=dt)
    cnt = n + dt(1.0) if mutation == "moments with count n + 1" else n
    if mode == "sgld":
        z = _noise(case, mode, variant, k, dt, mutation)
        noise = (dt(1.0) if mutation == "noise scaled by lr instead of lr^2" else lr) * z
        theta = theta0 + (-lr) * (g + noise)
        out.update(theta=theta, mean=(mean0 * cnt + theta) / (cnt + dt(1.0)), sq=(sq0 * cnt + theta ** 2) / (cnt + dt(1.0)))
        return out
    update, row = SWAG_STEPS[k]
    theta = theta0 - lr * g
    dev = np.asarray(s0["dev"], dtype=dt).copy()
    out.update(theta=theta, mean=mean0, sq=sq0, dev=dev)
    if update or mutation == "moments written on a non-update step":
        out["mean"] = (mean0 * cnt + theta) / (cnt + dt(1.0))
        out["sq"] = (sq0 * cnt + theta ** 2) / (cnt + dt(1.0))
        if update and row is not None:
            dev[row] = theta - (mean0 if mutation == "deviation against the old mean" else out["mean"])
    return out


def _ref_bbb(case, data, variant, k, s0, dt, mutation):
    spec, lr, alpha = case.spec, case.bbb_lr, case.alpha
    mu, rho = np.asarray(s0["mu"], dtype=dt), np.asarray(s0["rho"], dtype=dt)
    eps = _noise(case, "bbb", variant, k, dt, mutation)
    vec = case.prior_vec and mutation != "BBB prior vector ignored"
    pm = np.broadcast_to(np.asarray(data.pm_vec if vec else case.prior[0], dtype=dt), mu.shape)
    pr = np.broadcast_to(np.asarray(data.pr_vec if vec else case.prior[1], dtype=dt), mu.shape)
    sigma, sigma_p = _softplus(rho), _softplus(pr)
    w = mu + sigma * eps
    loss, g_loss = _gradient(w, data, spec, dt, mutation)
    lq = -0.5 * ((w - mu) / sigma) ** 2 - np.log(sigma) - _LOG_SQRT_2PI
    lp = -0.5 * ((w - pm) / sigma_p) ** 2 - np.log(sigma_p) - _LOG_SQRT_2PI
    kl = np.sum(lq) if mutation == "log q - log p without the prior term" else np.sum(lq) - np.sum(lp)
    cost = loss + alpha * kl
    d = w - mu
    sig = 1.0 / (1.0 + np.exp(-rho))
    g_mu = alpha * d / sigma ** 2
    g_rho = alpha * (-1.0 / sigma + d ** 2 / sigma ** 3) * sig
    if mutation == "BBB d rho with the wrong sign":
        g_rho = -g_rho
    g_w = g_loss + alpha * (-d / sigma ** 2 + (w - pm) / sigma_p ** 2)
    e = np.ones_like(eps) if mutation == "BBB rho update without eps" else eps
    sd_grad = e / (1.0 + np.exp(-rho)) * g_w + g_rho
    return {"mu": mu - lr * (g_mu + g_w), "rho": rho - lr * sd_grad, "w": w, "cost": np.array([cost, loss, kl], dtype=dt),
            "kl_abs": float(np.sum(np.abs(lq.astype(np.float64))) + np.sum(np.abs(lp.astype(np.float64))))}


def as_stored(out: dict) -> dict:
    """What a float32 device would leave of a reference step: every vector and scalar rounded to float32."""
    return {k: (v if k == "kl_abs" else np.asarray(v, dtype=np.float32)) for k, v in out.items()}


# ---------------------------------------------------------------- the comparison of one step
MOMENT_BOUND = 2.0 ** -20   # of (|m0| n + |theta1|) / (n + 1): at most four float32 roundings of intermediates no larger
#                             than that sum (2^-24 each), with room for a division good to 2.5 units in the last place
COST_SUM_BOUND = 2.0 ** -21  # of |loss| + |alpha kl|: cost = loss + alpha kl is one product and one sum (or one fused
#                              multiply-add) in float32, at most 2^-24 each of a magnitude below that sum; four times that


def _ratio(err, tol):
    err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(tol, 1e-300))))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} elements changed"


def _moment(got, m0, add, n, what):
    """|got - (m0 n + add) / (n + 1)| <= MOMENT_BOUND (|m0| n + |add|) / (n + 1), element by element, in float64."""
    got, m0, add = (np.asarray(a, dtype=np.float64) for a in (got, m0, add))
    err = np.abs(got - (m0 * n + add) / (n + 1.0))
    tol = MOMENT_BOUND * (np.abs(m0) * n + np.abs(add)) / (n + 1.0)
    bad = err > tol
    if bad.any():
        i = int(np.argmax(err / np.maximum(tol, 1e-300)))
        raise AssertionError(f"{what}: {int(bad.sum())} elements off the running mean of the stored theta, worst at {i}: "
                             f"error {err[i]:.3e} > {tol[i]:.3e}")
    return _ratio(err, tol)


def compare_step(case: StepCase, mode: str, k: int, s0: dict, got: dict, ref: dict, what: str = "") -> dict:
    """One step's result `got` (float32 vectors: a device's, or a stand-in's) against the float64 reference `ref` of the
    same step from the same state s0.  Raises AssertionError on the first bound missed; returns quantity -> error over
    tolerance.

    increments: got - s0 against ref - s0 per layer W and b block (close_blocks: 1e-4 of the block's reference scale, plus
        2^-23 max|state| of the block for the two float32 roundings of what is stored); BBB: mu, rho and the sampled w itself
    moments:    mean and sq_mean against the running mean of the STORED new theta, element by element (MOMENT_BOUND); the
        deviation row exactly theta1 - mean1 in float32; on a SWAG step without update, or without a row, nothing else moves
    losses:     1e-4 relative; BBB's log q - log p within 1e-5 of sum_e |log q_e| + |log p_e| (float32 terms summed in float64:
        about ten times a few units in the last place per term); cost = loss + alpha kl to float32 rounding"""
    spec, n = case.spec, float(case.n0 + k)
    rep = {}
    what = f"{what}{case.name} {mode} step {k}"
    for key in (("mu", "rho") if mode == "bbb" else ("theta",)):
        a0, a1 = s0[key].astype(np.float64), got[key].astype(np.float64)
        rep[f"d {key}"] = close_blocks(a1 - a0, np.asarray(ref[key], dtype=np.float64) - a0, spec, what=f"{what}: d {key}",
                                       state=np.maximum(np.abs(a0), np.abs(a1)))
    if mode == "bbb":
        rep["w"] = close_blocks(got["w"], ref["w"], spec, what=f"{what}: w", state=np.abs(got["w"]))
        c, r = np.asarray(got["cost"], dtype=np.float64), np.asarray(ref["cost"], dtype=np.float64)
        assert np.all(np.isfinite(c[:3])), f"{what}: cost {c}"
        rep["loss"] = _ratio(abs(c[1] - r[1]), 1e-4 * abs(r[1]))
        rep["kl"] = _ratio(abs(c[2] - r[2]), 1e-5 * ref["kl_abs"])
        alpha = float(np.float32(case.alpha))
        rep["cost"] = _ratio(abs(c[0] - (c[1] + alpha * c[2])), COST_SUM_BOUND * (abs(c[1]) + abs(alpha * c[2])))
        for q in ("loss", "kl", "cost"):
            assert rep[q] <= 1.0, f"{what}: {q}: cost triple {c[:3]} against {r} ({rep[q]:.3g} of the tolerance)"
        return rep
    rep["loss"] = _ratio(abs(float(got["loss"]) - float(ref["loss"])), 1e-4 * abs(float(ref["loss"])))
    assert rep["loss"] <= 1.0, f"{what}: loss {float(got['loss'])!r} against {float(ref['loss'])!r}"
    if mode == "sgd":
        return rep
    update, row = SWAG_STEPS[k] if mode == "swag" else (True, None)
    if update:
        th1 = got["theta"].astype(np.float64)
        rep["mean"] = _moment(got["mean"], s0["mean"], th1, n, f"{what}: mean")
        rep["sq_mean"] = _moment(got["sq"], s0["sq"], th1 * th1, n, f"{what}: sq_mean")
    else:
        _same_bits(got["mean"], s0["mean"], f"{what}: mean on a step without update")
        _same_bits(got["sq"], s0["sq"], f"{what}: sq_mean on a step without update")
    if mode == "swag":
        for r_ in range(s0["dev"].shape[0]):
            if update and r_ == row:
                _same_bits(got["dev"][r_], got["theta"].astype(np.float32) - got["mean"].astype(np.float32),
                           f"{what}: deviation row {r_} against float32(theta1) - float32(mean1)")
            else:
                _same_bits(got["dev"][r_], s0["dev"][r_], f"{what}: deviation row {r_}, which this step does not write")
    return rep


def old_parity_shapes():
    """The shapes the older step tests of tests/test_gpu_parity.py run, as cases of this table (for judging what they reach):
    name -> (StepCase, modes)."""
    t = lambda name, dims, acts, loss, batch, **kw: _c(name, dims, acts, loss, batch, aligned=True, **kw)
    return {
        "test_sgd_steps_match_oracle": (t("linreg", (1, 1), (LN,), MS, 64, gathered=True), ("sgd",)),
        "test_sgd_step_unfused_path": (t("wide_regression", (9, 16, 48), (R, LN), MS, 33), ("sgd",)),
        "test_swag_step_matches_oracle[tiny_cls]": (t("tiny_cls", (5, 7, 3), (R, SM), SC, 11), ("swag",)),
        "test_swag_step_matches_oracle[wide3]": (t("wide3", (64, 40, 24, 10), (R, R, SM), SC, 130), ("swag",)),
        "test_swag_step_matches_oracle[wide_regression]": (t("wide_regression", (9, 16, 48), (R, LN), MS, 33), ("swag",)),
        "test_sgld_step_injected_and_device_noise[tiny_cls]": (t("tiny_cls", (5, 7, 3), (R, SM), SC, 11), ("sgld",)),
        "test_sgld_step_injected_and_device_noise[wide3]": (t("wide3", (64, 40, 24, 10), (R, R, SM), SC, 130), ("sgld",)),
        "test_sgld_step_injected_and_device_noise[many_classes]": (t("many_classes", (12, 20, 40), (T, SM), SC, 70), ("sgld",)),
        "test_sgld_step_injected_and_device_noise[wide_regression]": (t("wide_regression", (9, 16, 48), (R, LN), MS, 33), ("sgld",)),
        "test_bbb_step_matches_oracle[tiny_cls]": (t("tiny_cls", (5, 7, 3), (R, SM), SC, 11), ("bbb",)),
        "test_bbb_step_matches_oracle[reg3]": (t("reg3", (4, 6, 6, 2), (T, G, LN), MS, 37), ("bbb",)),
        "test_bbb_step_matches_oracle[wide3]": (t("wide3", (64, 40, 24, 10), (R, R, SM), SC, 130), ("bbb",)),
        "test_bbb_step_matches_oracle[many_classes]": (t("many_classes", (12, 20, 40), (T, SM), SC, 70), ("bbb",)),
        "test_list_valued_priors_bbb_and_hmc": (t("tiny_cls", (5, 7, 3), (R, SM), SC, 11, prior_vec=True), ("bbb",)),
        "test_dense_case[wg_sgd_s1]": (t("wg_sgd_s1", (20, 16, 4), (R, SM), SC, 30), ("sgd",)),
    }
