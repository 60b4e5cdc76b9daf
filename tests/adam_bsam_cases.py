"""The case table of the eager ADAM, VADAM and BSAM steps and the comparison both step tests share (a plain module).

These steps do not run k_wgrad_all.  A fused step (last layer of at most 32 units) runs k_wgrad_adam<S>, with a second
MFMA chain for the squared per-example gradients, or k_wgrad_bsam<S, 0> and k_wgrad_bsam<S, 1>; an unfused ADAM / VADAM step
runs k_dense_bwd_weight_sq per layer and k_adam_update, an unfused BSAM step k_dense_bwd_weight per layer and pass with
k_bsam_ascent and k_bsam_update; k_vadam_perturb / k_bsam_perturb draw the perturbation.  This module restates which of them
a (case, kind) launches and with which S (`expected_ab_launches`, on top of dense_cases.expected_launches), names the cells
of the coverage table (`CELLS`, `reached_cells`), lists cases that reach every cell with every kind, builds their data
(dense_cases.case_data plus a starting state that is not zero), restates one step of each kind in a chosen dtype on top of
adam_checks.grad_moments (per-row oracle gradients: not the (A o A)^T (Delta o Delta) identity the kernels use) and the
arithmetic of bsam_checks.BsamRef, with the wrong variants the sensitivity check needs (`ref_step`, `MUTATIONS`), and holds
the comparison of one step (`compare_step`).  tests/test_adam_bsam_dispatch_table.py pins all of it to the source and to
AdamRef / BsamRef on the CPU; tests/test_gpu_adam_bsam_matrix.py runs the cases on the device.

A case takes three chained steps, each from the device's previous state, with different hyper-parameters (`adam_hyper`,
`bsam_hyper`): step 0 the reference VADAM driver's lr and betas (BSAM: its own driver's setting), step 1 a small beta_2
(0.5; 0 on the one-layer cases), so that the squared-gradient mean s and not v0 decides v and the update (BSAM: the "sharp"
setting), step 2 decay != 0 and a denom_eps other than 1e-3 (BSAM: "sharp" with beta_1 = beta_2 = 0.5 and a larger rho).
VADAM's decay = denom_eps = lam / N on every step.  The epoch (BSAM: the Philox step) differs from step to step.

The elementwise check of the one-layer cases.  After the beta_2 = 0 step v IS s, a sum of non-negative terms, so every
element can be held to a relative bound of its own.  Its tolerance is measured, not chosen: the elementwise relative error
of the identity (`identity_moments`) evaluated in float32 against grad_moments in float64 on these very inputs is at most
2.01e-06 over the five one-layer cases (3.9e-07 f_s4_self_l1, 2.01e-06 u_d99, 3.3e-07 u_d165_mse, 1.14e-06 u_g16_plain,
1.06e-06 u_g16_self; tests/test_adam_bsam_dispatch_table.py measures it again and holds it to V_ELEMENTWISE_MEASURED =
2.1e-06); with the project's margin of 4 for the kernel's other summation order the bound is V_ELEMENTWISE_TOL = 8.4e-06."""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import adam_checks as ac
import bsam_checks as bc
from dense_cases import DenseCase, batch_rows, can_fuse, case_data, cdiv, expected_launches, pick_waves, wgrad_steps, wgrad_tiles
from head_cases import close_blocks
from oracle import mlp as o_mlp
from oracle import philox as o_philox
from step_cases import CASES as STEP_CASES

# ---------------------------------------------------------------- the rules (csrc/pyz_api.hip, pyz_gemm.h, pyz_kernels.h)
KINDS = ("adam", "vadam", "bsam")
STREAM = {"vadam": 5, "bsam": 6}            # PYZ_STREAM_VADAM, PYZ_STREAM_BSAM
VARIANTS = {"adam": ("plain",), "vadam": ("injected", "device"), "bsam": ("injected", "device")}
PERTURB_KERNEL = {"vadam": "k_vadam_perturb", "bsam": "k_bsam_perturb"}
PER_THREAD = {"k_adam_update": 1, "k_bsam_ascent": 1, "k_bsam_update": 1, "k_vadam_perturb": 4, "k_bsam_perturb": 4}
SS = (1, 2, 4, 8, 16)
GROUPS = (16, 4, 1)                         # k_dense_bwd_weight_sq: pyz_wgrad_steps<16>, <4>, <1>, in this order
N_STEPS = 3
F32 = np.float32


def wgrad_adam_expr(S: int) -> str:         # launch_wgrad_adam: the arms of switch (S) (default: 16)
    return f"k_wgrad_adam<{S}>"


def wgrad_bsam_expr(S: int, phase: int) -> str:   # launch_wgrad_bsam (the probe reports it without the macro's parentheses)
    return f"k_wgrad_bsam<{S}, {phase}>"


def wgrad_lds_bytes(S: int) -> int:         # both launchers: no LDS with one wave, else 4096 bytes per wave
    return 0 if S == 1 else S * 4096


def update_grid(kernel: str, D: int) -> int:
    """Blocks of 256 threads: cdiv(D, 256) for the one-element kernels, cdiv(cdiv(D, 4), 256) for the perturbations."""
    return cdiv(cdiv(D, PER_THREAD[kernel]), 256)


def wave_ranges(steps: int, S: int):
    return [((steps * w) // S, (steps * (w + 1)) // S) for w in range(S)]


def groups_of(n: int) -> set:
    """The groups of k_dense_bwd_weight_sq a wave of n steps runs: 16 while 16 steps are left, then 4, then 1."""
    return {G for G, on in ((16, n >= 16), (4, n % 16 >= 4), (1, n % 4 >= 1)) if on}


class AbCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str
    batch: int
    gathered: bool = False
    aligned: bool = False    # state buffers 16-byte aligned (else 4 bytes off)
    data_seed: int = 0
    e0: int = 3              # the first step's epoch is e0, the others follow `EPOCH_OF`; BSAM / VADAM: Philox step e0 + k
    seed: int = 11           # Philox seed
    n_vadam: float = 32.0    # VADAM's N: small, so that decay = denom_eps = lam / N and the perturbation all show
    n_bsam: float = 32768.0  # BSAM's N enters the perturbation only; large, see `box_muller_share`

    @property
    def spec(self) -> o_mlp.MLPSpec:
        return o_mlp.MLPSpec(self.dims, self.acts, self.loss)

    @property
    def D(self) -> int:
        return self.spec.n_params

    @property
    def L(self) -> int:
        return len(self.dims) - 1

    @property
    def fused(self) -> bool:
        return can_fuse(self.dims)

    @property
    def dense(self) -> DenseCase:
        return DenseCase(self.name, self.dims, self.acts, self.loss, 1, self.batch, self.gathered, False, {}, True, self.data_seed)

    @property
    def max_batch(self) -> int:
        return self.batch + 3


class SqLaunch(NamedTuple):
    layer: int
    K: int
    N: int
    S: int
    gather: str        # "none" or "self"
    waves: tuple       # steps of each wave
    groups: frozenset  # the G of pyz_wgrad_steps<G, GATHER, true> some wave of the launch runs


class AbLaunches(NamedTuple):
    perturb: tuple     # the perturbation kernel (VADAM: the launch of vadam_perturb, a call of its own)
    sequence: tuple    # the weight-gradient and update kernels of the step in launch order, as KernelProbe reports them
    S: int             # waves of k_wgrad_adam / k_wgrad_bsam (0 when unfused)
    gather: str        # "none", "copy" (layer 0 reads the forward's batch copy) or "self" (gathers through row_idx)
    sq: tuple          # unfused ADAM / VADAM: one SqLaunch per layer, in launch order


def expected_ab_launches(case: AbCase, kind: str) -> AbLaunches:
    """pyz_adam_step: fused = launch_loss_backward(..., &a) ends in launch_wgrad_adam, one k_wgrad_adam<S>; else
    launch_backward(..., m->grad2) runs pyz_launch_bwd_weight_sq per layer, last layer first, and k_adam_update follows.
    pyz_vadam_perturb: k_vadam_perturb.  pyz_bsam_step: k_bsam_perturb; fused = launch_bsam_pass twice, ending in
    k_wgrad_bsam<S, 0> and k_wgrad_bsam<S, 1>; else launch_loss_backward (k_dense_bwd_weight per layer) with k_bsam_ascent
    and again with k_bsam_update.  S = pyz_pick_waves(tiles of all layers, (batch + 1) / 2), one chain.  Layer 0 reads the
    batch copy `xb` only with row_idx and L > 1 ("copy"); a gathered one-layer model, and layer 0 of an unfused one,
    gathers for itself ("self")."""
    la = expected_launches(case.dense)
    perturb = (PERTURB_KERNEL[kind],) if kind in PERTURB_KERNEL else ()
    gathers = {w.gather for w in la.wgrad} - {""}
    assert len(gathers) <= 1
    gather = gathers.pop() if gathers else "none"
    if case.fused:
        tiles = sum(wgrad_tiles(K, N) for K, N in zip(case.dims[:-1], case.dims[1:]))
        S, _ = pick_waves(tiles, wgrad_steps(case.batch))
        assert la.wgrad[0].S == S
        seq = (wgrad_bsam_expr(S, 0), wgrad_bsam_expr(S, 1)) if kind == "bsam" else (wgrad_adam_expr(S),)
        return AbLaunches(perturb, seq, S, gather, ())
    assert [w.kernel for w in la.wgrad] == ["k_dense_bwd_weight"] * case.L
    if kind == "bsam":
        one = ("k_dense_bwd_weight",) * case.L
        return AbLaunches(perturb, one + ("k_bsam_ascent",) + one + ("k_bsam_update",), 0, gather, ())
    sq = []
    for l, w in zip(range(case.L - 1, -1, -1), la.wgrad):
        (K, N), = w.layers
        S, _ = pick_waves(wgrad_tiles(K, N), wgrad_steps(case.batch))   # pyz_launch_bwd_weight_sq
        assert S == w.S
        waves = tuple(e - s for s, e in wave_ranges(wgrad_steps(case.batch), S))
        sq.append(SqLaunch(l, K, N, S, w.gather or "none", waves, frozenset().union(*[groups_of(n) for n in waves])))
    return AbLaunches(perturb, ("k_dense_bwd_weight_sq",) * case.L + ("k_adam_update",), 0, gather, tuple(sq))


# ---------------------------------------------------------------- the coverage table
CELLS = frozenset(
    [f"{k} S={S}" for k in KINDS for S in SS] +
    [f"{k} gather={g}" for k in KINDS for g in ("none", "copy", "self")] +
    [f"k_dense_bwd_weight_sq G={G} gather={g}" for G in GROUPS for g in ("none", "self")] +
    [f"unfused {k} D%4={r}" for k in PERTURB_KERNEL.values() for r in range(4)] +
    [f"unfused {k} D spans more than one 256-thread block" for k in ("k_adam_update", "k_bsam_ascent", "k_bsam_update")] +
    [f"{k} {v} noise" for k in PERTURB_KERNEL for v in ("injected", "device")] +
    ["odd batch", "batch = 1", "batch = 2", "K + 1 = 32", "K + 1 = 33", "ragged N",
     "more than one column tile on the fused path", "more than one row tile and more than one column tile in one layer",
     "state buffers 16-byte aligned", "state buffers 4 bytes off 16-byte alignment"])


def reached_cells(case: AbCase, kinds=KINDS) -> set:
    """The cells a case reaches with the given kinds, from its shape and `expected_ab_launches` alone."""
    cells = set()
    for k in kinds:
        la = expected_ab_launches(case, k)
        cells.add(f"{k} gather={la.gather}")
        if case.fused:
            cells.add(f"{k} S={la.S}")
        else:
            for q in la.sq:
                if q.layer == 0:      # the layer whose rows a gather reaches
                    cells |= {f"k_dense_bwd_weight_sq G={G} gather={q.gather}" for G in q.groups}
            if k in PERTURB_KERNEL:
                cells.add(f"unfused {PERTURB_KERNEL[k]} D%4={case.D % 4}")
            if case.D > 256:
                names = ("k_bsam_ascent", "k_bsam_update") if k == "bsam" else ("k_adam_update",)
                cells |= {f"unfused {n} D spans more than one 256-thread block" for n in names}
        if k in PERTURB_KERNEL:
            cells |= {f"{k} {v} noise" for v in VARIANTS[k]}
    cells.add("state buffers 16-byte aligned" if case.aligned else "state buffers 4 bytes off 16-byte alignment")
    if case.batch % 2:
        cells.add("odd batch")
    if case.batch in (1, 2):
        cells.add(f"batch = {case.batch}")
    for K, N in zip(case.dims[:-1], case.dims[1:]):
        if K + 1 in (32, 33):
            cells.add(f"K + 1 = {K + 1}")
        if N % 32:
            cells.add("ragged N")
        if case.fused and N > 32:
            cells.add("more than one column tile on the fused path")
        if K + 1 > 32 and N > 32:
            cells.add("more than one row tile and more than one column tile in one layer")
    return cells & CELLS


R, T, G, LN, SM = "relu", "tanh", "sigmoid", "linear", "softmax"
SC, MS = "scce", "mse"


def _c(name, dims, acts, loss, batch, **kw):
    return AbCase(name, tuple(dims), tuple(acts), loss, batch, **kw)


CASES = [_c(c.name, c.dims, c.acts, c.loss, c.batch, gathered=c.gathered, aligned=c.aligned, data_seed=c.data_seed)
         for c in STEP_CASES] + [
    # ---- what the thirteen shapes of the step matrix leave: the peeled odd row as the whole reduction (batch 1: s = g^2),
    # one whole MFMA step (batch 2); several row and column tiles in one layer of a fused model; a wave of 21 steps in
    # k_dense_bwd_weight_sq (S = 16 by the cap: groups of 16, 4 and 1), rows contiguous and gathered
    _c("f_b1", (20, 16, 4), (R, SM), SC, 1, data_seed=1),
    _c("f_b2", (20, 16, 4), (R, SM), SC, 2, aligned=True),
    _c("f_tiles_2x3", (33, 65, 10), (T, SM), SC, 45),
    _c("u_g16_plain", (4, 33), (SM,), SC, 671),
    _c("u_g16_self", (3, 33), (LN,), MS, 671, gathered=True, aligned=True),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"
ONE_LAYER = tuple(c.name for c in CASES if c.L == 1)


# ---------------------------------------------------------------- the hyper-parameters of the three steps
EPOCH_OF = (997, -1, 2)   # added to e0: the epochs 1000, 2, 5 by default


def adam_hyper(case: AbCase, kind: str, k: int) -> dict:
    """lr, beta_1, beta_2, epoch, denom_eps, decay of step k (VADAM: and lam, N with decay = denom_eps = lam / N)."""
    h = (dict(lr=0.01, beta_1=0.9, beta_2=0.999),                                        # the reference VADAM driver's
         dict(lr=0.0625, beta_1=0.5, beta_2=0.0 if case.L == 1 else 0.5),                 # s, not v0, decides v
         dict(lr=0.03125, beta_1=0.75, beta_2=0.875))[k].copy()
    h["epoch"] = case.e0 + EPOCH_OF[k]
    if kind == "vadam":
        lam = (0.5, 0.5, 2.0)[k]
        h.update(lam=lam, num_data=case.n_vadam, denom_eps=lam / case.n_vadam, decay=lam / case.n_vadam)
    else:
        h.update(denom_eps=(1e-3, 1e-3, 0.015625)[k], decay=(0.0, 0.0, 0.03125)[k])
    return h


def bsam_hyper(case: AbCase, k: int) -> dict:
    """Both settings of bsam_checks.SETTINGS, and the sharp one with both betas at 0.5 and five times the ascent."""
    h = (bc.SETTINGS["driver"], bc.SETTINGS["sharp"],
         dict(bc.SETTINGS["sharp"], lr=0.03125, beta_1=0.5, beta_2=0.5, lam=0.25, rho=0.05))[k]
    return dict(h, num_data=case.n_bsam)


def philox_step(case: AbCase, k: int) -> int:
    return case.e0 + k


# ---------------------------------------------------------------- data
class AbData(NamedTuple):
    x: np.ndarray
    y: np.ndarray
    idx: Optional[np.ndarray]
    rows: np.ndarray         # the batch rows and their targets
    ys: np.ndarray
    theta0: np.ndarray       # float32 (D)
    m0: np.ndarray           # of the size of the gradient
    v0_adam: np.ndarray      # positive, of the size of the float64 s, floored per block
    v0_bsam: np.ndarray      # uniform in [0.5, 2]


V0_FLOOR = 0.01              # of a block's largest s


def blocks(spec):
    for l, ((ko, bo), K, N) in enumerate(zip(spec.offsets(), spec.dims[:-1], spec.dims[1:])):
        yield f"W{l}", slice(ko, ko + K * N)
        yield f"b{l}", slice(bo, bo + N)


_DATA = {}


def ab_data(case: AbCase) -> AbData:
    """dense_cases.case_data (edges weighted) and a starting state that is not zero: m0 of either sign, element by element
    0.5 to 1.5 times |g| + a tenth of the block's rms; ADAM's v0 = s (the float64 squared-gradient mean at theta0) times a factor in [0.5, 1.5], not below
    V0_FLOOR of the block's largest s -- where a unit is dead s is zero, and without the floor m^ / eps of those elements
    would be the scale every other element of the block is judged on; BSAM's v0 uniform in [0.5, 2]."""
    if case.name in _DATA:
        return _DATA[case.name]
    x, y, idx, thetas = case_data(case.dense)
    rows, ys = batch_rows(case.dense, x, y, idx)
    theta0 = thetas[0]
    D, spec = theta0.size, case.spec
    rng = np.random.default_rng(sum(map(ord, case.name)) + 7919 * (case.data_seed + 1))
    _, g, s = ac.grad_moments(theta0, rows, ys, spec)
    m0, v0 = np.empty(D), np.empty(D)
    g_rms = float(np.sqrt(np.mean(g * g)))
    for _, sl in blocks(spec):
        rms = max(float(np.sqrt(np.mean(g[sl] ** 2))), 1e-3 * g_rms)
        m0[sl] = (np.abs(g[sl]) + 0.1 * rms) * rng.uniform(0.5, 1.5, size=g[sl].size) * rng.choice([-1.0, 1.0], size=g[sl].size)
        v0[sl] = np.maximum(s[sl], V0_FLOOR * max(s[sl].max(), 1e-6 * s.max())) * rng.uniform(0.5, 1.5, size=g[sl].size)
    v0_bsam = rng.uniform(0.5, 2.0, size=D)
    _DATA[case.name] = AbData(x, y, idx, rows, ys, theta0, m0.astype(F32), v0.astype(F32), v0_bsam.astype(F32))
    return _DATA[case.name]


def initial_state(kind: str, data: AbData) -> dict:
    if kind == "bsam":      # BSAM's m averages g2 + lam theta: the state of a chain that has run at the sharp setting's lam
        m0 = (data.m0.astype(np.float64) + bc.SETTINGS["sharp"]["lam"] * data.theta0.astype(np.float64)).astype(F32)
        return {"theta": data.theta0.copy(), "m": m0, "v": data.v0_bsam.copy()}
    return {"theta": data.theta0.copy(), "m": data.m0.copy(), "v": data.v0_adam.copy()}


def injected_noise(case: AbCase, kind: str, variant: str, k: int):
    """The float32 vector a step is given as eps (None: the device draws it, or the kind has no noise)."""
    if kind not in STREAM or variant == "device":
        return None
    return o_philox.normal(case.seed, STREAM[kind], philox_step(case, k), case.D).astype(F32)


# ---------------------------------------------------------------- one step, restated (any dtype, wrong variants)
S_MUT = ("s as the square of the mean gradient", "s not divided by B", "s divided by max_batch instead of the batch",
         "bias row of the last layer missing from s", "last row of W0 missing from s")
MUTATIONS = {   # name -> the kinds it applies to
    S_MUT[0]: ("adam", "vadam"),
    S_MUT[1]: ("adam", "vadam"),
    S_MUT[2]: ("adam", "vadam"),
    S_MUT[3]: ("adam", "vadam"),
    S_MUT[4]: ("adam", "vadam"),
    "last layer's bias gradient scaled by 1.001": KINDS,
    "last row of W0's gradient dropped": KINDS,
    "bias correction with epoch + 1": ("adam", "vadam"),
    "decay taken on the unperturbed weight": ("vadam",),
    "denom_eps left at 1e-3": ("vadam",),
    "perturbation with sqrt(N v + lam)": ("vadam",),
    "noise drawn for element e + 1": ("vadam", "bsam"),
    "noise of the last 4-group zero": ("vadam", "bsam"),
    "BSAM ascent with g1 / sqrt(v)": ("bsam",),
    "BSAM update with g2 where g1 belongs": ("bsam",),
    "BSAM update with sqrt of the unscaled v": ("bsam",),
    "BSAM update with lam + gam dropped": ("bsam",),
    "BSAM update with m from g1": ("bsam",),
}


def mutation_applies(case: AbCase, kind: str, mutation: str) -> bool:
    if kind not in MUTATIONS[mutation]:
        return False
    if case.batch == 1 and mutation in S_MUT[:2]:
        return False      # one example: the mean of the squares IS the square of the mean, and B = 1 divides nothing
    return True


def _noise(case: AbCase, kind: str, variant: str, k: int, dt, mutation):
    """The N(0, 1) vector of a step as the arithmetic sees it: the injected float32 values, or (device) the float64 draws."""
    D = case.D
    z = o_philox.normal(case.seed, STREAM[kind], philox_step(case, k), D + 1)
    z = z[1:] if mutation == "noise drawn for element e + 1" else z[:D]
    if variant == "injected":
        z = z.astype(F32)
    z = z.astype(dt)
    if mutation == "noise of the last 4-group zero":
        z[4 * ((D - 1) // 4):] = 0
    return z


def _mutate_grad(g, spec, dt, mutation):
    if mutation == "last layer's bias gradient scaled by 1.001":
        bo = spec.offsets()[-1][1]
        g[bo:] = g[bo:] * dt(1.001)
    if mutation == "last row of W0's gradient dropped":
        K, N = spec.dims[0], spec.dims[1]
        g[(K - 1) * N:K * N] = 0
    return g


def moments(theta, rows, ys, spec, dt=np.float64):
    """(loss, g, s) in dt: float64 is adam_checks.grad_moments itself; float32 is the same row-by-row sum with every
    operation in float32."""
    if dt == np.float64:
        return ac.grad_moments(theta, rows, ys, spec)
    loss = o_mlp.loss_and_grad(theta, rows, ys, spec, dt)[0]
    g, s = np.zeros(spec.n_params, dtype=dt), np.zeros(spec.n_params, dtype=dt)
    for i in range(len(rows)):
        gi = o_mlp.loss_and_grad(theta, rows[i:i + 1], ys[i:i + 1], spec, dt)[1]
        g += gi
        s += gi * gi
    return loss, g / dt(len(rows)), s / dt(len(rows))


def identity_moments(theta, rows, ys, spec, dt=np.float64):
    """adam_checks.identity_moments -- g = A^T Delta, s = (A o A)^T ((B Delta) o (B Delta)) / B, what the kernels compute --
    with every operation in dt (float64: bit-equal to it)."""
    acts, _ = o_mlp.forward(theta, rows, spec, dt)
    out, B = acts[-1], len(rows)
    if spec.loss == "scce":
        delta = out.copy()
        delta[np.arange(B), np.asarray(ys).reshape(-1).astype(np.int64)] -= dt(1.0)
        delta /= dt(B)
    else:
        delta = dt(2.0) * (out - np.asarray(ys, dtype=dt).reshape(out.shape)) / dt(B * out.shape[1])
        delta = delta * o_mlp._act_grad_from_output(out, spec.acts[-1])
    ws = o_mlp.unpack(np.asarray(theta, dtype=dt), spec)
    gs, ss = [None] * spec.n_layers, [None] * spec.n_layers
    for l in range(spec.n_layers - 1, -1, -1):
        a = np.concatenate([acts[l], np.ones((B, 1), dtype=dt)], axis=1)
        gs[l] = (a.T @ delta).reshape(-1)
        ss[l] = ((a * a).T @ ((dt(B) * delta) ** 2)).reshape(-1) / dt(B)
        if l > 0:
            delta = (delta @ ws[l][0].T) * o_mlp._act_grad_from_output(acts[l], spec.acts[l - 1])
    return np.concatenate(gs), np.concatenate(ss)


def _mutate_s(s, g, case, dt, mutation):
    spec, B = case.spec, case.batch
    if mutation == S_MUT[0]:
        return g * g
    if mutation == S_MUT[1]:
        return s * dt(B)
    if mutation == S_MUT[2]:
        return s * dt(B) / dt(case.max_batch)
    s = s.copy()
    if mutation == S_MUT[3]:
        s[spec.offsets()[-1][1]:] = 0
    if mutation == S_MUT[4]:
        K, N = spec.dims[0], spec.dims[1]
        s[(K - 1) * N:K * N] = 0
    return s


def ref_step(case: AbCase, kind: str, state: dict, k: int, dtype=np.float64, mutation=None, variant=None, pert=None) -> dict:
    """Step k of `kind` from `state` (theta, m, v) in `dtype`, with `mutation` one of the wrong variants above: the
    arithmetic of AdamRef.perturb / AdamRef.step and BsamRef.step (tests/test_adam_bsam_dispatch_table.py holds the
    float64 version bit-equal to them).  VADAM: "pert" is theta behind the perturbation; the update then starts from
    `pert` when it is given (the device's own perturbed weights), so that each launch is judged on its own.  BSAM: "asc"
    is the ascent point theta + eps / (N v) + rho g1 / v, which the update leaves from and never undoes."""
    dt, spec = dtype, case.spec
    data = ab_data(case)
    variant = variant or VARIANTS[kind][0]
    theta, m, v = (np.asarray(state[q], dtype=dt) for q in ("theta", "m", "v"))
    if kind == "bsam":
        return _ref_bsam(case, data, variant, k, theta, m, v, dt, mutation)
    h = adam_hyper(case, kind, k)
    out = {}
    w = theta
    if kind == "vadam":
        eps = _noise(case, kind, variant, k, dt, mutation)
        n, lam = dt(F32(h["num_data"])), dt(F32(h["lam"]))
        den = n * v + lam if mutation == "perturbation with sqrt(N v + lam)" else n * (v + lam)
        out["pert"] = theta + eps / np.sqrt(den)
        w = out["pert"] if pert is None else np.asarray(pert, dtype=dt)
    loss, g, s = moments(w, data.rows, data.ys, spec, dt)
    g = _mutate_grad(np.array(g, dtype=dt), spec, dt, mutation)
    s = _mutate_s(np.asarray(s, dtype=dt), g, case, dt, mutation)
    epoch = h["epoch"] + (mutation == "bias correction with epoch + 1")
    eps_d = 1e-3 if mutation == "denom_eps left at 1e-3" else h["denom_eps"]
    c = {q: dt(x) for q, x in ac.scalars(h["lr"], h["beta_1"], h["beta_2"], epoch, eps_d, h["decay"]).items()}
    wd = theta if mutation == "decay taken on the unperturbed weight" else w
    m1 = c["b1"] * m + c["c1"] * (g + c["decay"] * wd)
    v1 = c["b2"] * v + c["c2"] * s
    mh, vh = m1 / c["bc1"], v1 / c["bc2"]
    out.update(theta=w - c["lr"] * mh / (np.sqrt(vh) + c["eps"]), m=m1, v=v1, loss=np.array([loss], dtype=dt))
    return out


def _ref_bsam(case, data, variant, k, theta, m, v, dt, mutation):
    spec, h = case.spec, bsam_hyper(case, k)
    c = {q: dt(x) for q, x in bc.scalars(**h).items()}

    def grad(th):
        loss, g = o_mlp.loss_and_grad(th.astype(np.float64), data.rows, data.ys, spec)[:2]
        return float(loss), _mutate_grad(np.asarray(g).astype(dt), spec, dt, mutation)

    eps = _noise(case, "bsam", variant, k, dt, mutation)
    theta = theta + eps * (c["inv_n"] / v)
    l1, g1 = grad(theta)
    theta = theta + c["rho"] * (g1 / (np.sqrt(v) if mutation == "BSAM ascent with g1 / sqrt(v)" else v))
    asc = theta
    l2, g2 = grad(theta)
    m1 = c["b1"] * m + c["c1"] * ((g1 if mutation == "BSAM update with m from g1" else g2) + c["lam"] * theta)
    vb = c["b2"] * v
    gv = g2 if mutation == "BSAM update with g2 where g1 belongs" else g1
    shift = gv if mutation == "BSAM update with lam + gam dropped" else gv + c["lam"] + c["gam"]
    root = np.sqrt(v) if mutation == "BSAM update with sqrt of the unscaled v" else np.sqrt(vb)
    v1 = vb + c["c2"] * (root * np.abs(shift))
    return {"theta": theta - c["lr"] * m1 / v1, "m": m1, "v": v1, "asc": asc, "loss": np.array([l1, l2], dtype=dt)}


def as_stored(out: dict) -> dict:
    """What a float32 device would leave of a reference step: every vector rounded to float32 (the ascent point is not
    stored: compare_step takes it from theta, m and v)."""
    return {q: np.asarray(a, dtype=F32) for q, a in out.items() if q != "asc"}


# ---------------------------------------------------------------- the comparison of one step
REL = 1e-4                         # the project's tolerance, per layer block
V_ELEMENTWISE_MEASURED = 2.1e-6     # float32 identity against float64 per-row moments, elementwise relative, one-layer cases
V_ELEMENTWISE_TOL = 4.0 * V_ELEMENTWISE_MEASURED
UPDATE_ROUNDINGS = {"adam": 2.0, "vadam": 2.0, "bsam": 3.0}   # close_blocks allows 2^-24 max|state| per float32 rounding of
#                                    what is stored and counts two; a BSAM step stores theta three times between theta0 and
#                                    theta1 (k_bsam_perturb, the ascent, the update), each rounded to float32
ASC_ROUNDINGS = 8.0              # the allowance of "asc" is 2^-20 max|theta| of the block: three float32 roundings of
#                                    weight-sized numbers lie between theta0 and the stored theta1 (+ perturbation, + ascent,
#                                    - update: 2^-24 max|theta| each), and 2^-20 is four times their worst case with room for
#                                    the float32 lr m1 / v1 the device subtracted (MOMENT_BOUND's reasoning in step_cases.py)
BOX_MULLER_ABS = 3.2e-5           # the device's float32 Box-Muller against the oracle's float64 one, per normal
#                                    (tests/test_gpu_adam_vadam.py::test_vadam_philox_perturbation: 8 x the 4e-6 of DESIGN 8)


def _ratio(err, tol):
    err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(tol, 1e-300))))


def ascent_point(case: AbCase, k: int, got: dict):
    """BSAM stores theta1 = asc - lr m1 / v1 and never the ascent point: asc = theta1 + lr m1 / v1, in float64 from the
    stored vectors and the float32 lr."""
    lr = np.float64(F32(bsam_hyper(case, k)["lr"]))
    return got["theta"].astype(np.float64) + lr * got["m"].astype(np.float64) / got["v"].astype(np.float64)


def is_elementwise_step(case: AbCase, kind: str, k: int) -> bool:
    return kind != "bsam" and case.L == 1 and adam_hyper(case, kind, k)["beta_2"] == 0.0


def compare_step(case: AbCase, kind: str, k: int, s0: dict, got: dict, ref: dict, what: str = "") -> dict:
    """One step's result `got` (float32 vectors: a device's, or a stand-in's) against the float64 reference `ref` of the
    same step from the same state s0.  Raises AssertionError on the first bound missed; returns quantity -> error over
    tolerance.

    update:  theta1 - theta0 (VADAM: theta1 - the perturbed weights the update started from, and "pert" = those - theta0)
        per layer W and b block: close_blocks at 1e-4 of the block's reference scale plus 2^-23 max|state| of the block for
        the two float32 roundings of what is stored
    m, v:    per block at 1e-4 of the block's reference scale
    asc:     BSAM's ascent point (`ascent_point`) less theta0, like the update
    v elementwise: the one-layer cases after the beta_2 = 0 step, |v - s| <= V_ELEMENTWISE_TOL s, element by element
    loss:    1e-4 relative (BSAM: both)"""
    spec = case.spec
    what = f"{what}{case.name} {kind} step {k}"
    rep = {}
    t0 = s0["theta"].astype(np.float64)
    t1 = got["theta"].astype(np.float64)
    base = t0
    if kind == "vadam":
        base = got["pert"].astype(np.float64)
        rep["pert"] = close_blocks(base - t0, np.asarray(ref["pert"], dtype=np.float64) - t0, spec, REL, f"{what}: pert",
                                   state=np.maximum(np.abs(t0), np.abs(base)))
    rep["update"] = close_blocks(t1 - base, np.asarray(ref["theta"], dtype=np.float64) - base, spec, REL, f"{what}: update",
                                 state=UPDATE_ROUNDINGS[kind] / 2.0 * np.maximum(np.abs(base), np.abs(t1)))
    rep["m"] = close_blocks(got["m"], ref["m"], spec, REL, f"{what}: m")
    rep["v"] = close_blocks(got["v"], ref["v"], spec, REL, f"{what}: v")
    if kind == "bsam":
        asc = ascent_point(case, k, got)
        rep["asc"] = close_blocks(asc - t0, np.asarray(ref["asc"], dtype=np.float64) - t0, spec, REL, f"{what}: asc",
                                  state=ASC_ROUNDINGS * np.maximum(np.abs(t0), np.maximum(np.abs(asc), np.abs(t1))))
    if is_elementwise_step(case, kind, k):
        s, v = np.asarray(ref["v"], dtype=np.float64), got["v"].astype(np.float64)
        assert np.all(s > 0), f"{what}: an element of s is zero"
        rel = np.abs(v - s) / s
        rep["v elementwise"] = float(rel.max() / V_ELEMENTWISE_TOL)
        assert rep["v elementwise"] <= 1.0, (f"{what}: v = s elementwise: relative error {rel.max():.3e} at {int(rel.argmax())} "
                                             f"(got {v[rel.argmax()]:.6e}, ref {s[rel.argmax()]:.6e}) > {V_ELEMENTWISE_TOL:g}")
    lg, lr_ = np.asarray(got["loss"], dtype=np.float64).reshape(-1), np.asarray(ref["loss"], dtype=np.float64).reshape(-1)
    assert lg.shape == lr_.shape and np.all(np.isfinite(lg)), f"{what}: loss {lg}"
    rep["loss"] = _ratio(np.abs(lg - lr_), REL * np.abs(lr_))
    assert rep["loss"] <= 1.0, f"{what}: loss {lg} against {lr_}"
    return rep


def box_muller_share(case: AbCase, kind: str, k: int, s0: dict, ref: dict) -> float:
    """The device draws its normals with a float32 Box-Muller that differs from the oracle's float64 one by at most
    BOX_MULLER_ABS per normal, and the reference of the device-noise variant is fed the oracle's.  Largest share of a
    block's tolerance that difference can take in the one quantity that holds the perturbation itself: VADAM's "pert"
    (eps / sqrt(N (v + lam))) and BSAM's "asc" (eps / (N v) + rho g1 / v).  Everything behind it sees the shift only
    through the gradient at a point moved by a few 1e-5 of the perturbation."""
    t0, v = s0["theta"].astype(np.float64), s0["v"].astype(np.float64)
    if kind == "vadam":
        h = adam_hyper(case, kind, k)
        gain = 1.0 / np.sqrt(h["num_data"] * (v + h["lam"]))
        inc = np.asarray(ref["pert"], dtype=np.float64) - t0
    else:
        gain = (1.0 / bsam_hyper(case, k)["num_data"]) / v
        inc = np.asarray(ref["asc"], dtype=np.float64) - t0
    floor = 1e-3 * np.abs(inc).max()
    worst = 0.0
    for _, sl in blocks(case.spec):
        tol = REL * max(np.abs(inc[sl]).max(), floor) + 2.0 ** -23 * np.abs(t0[sl]).max()
        worst = max(worst, BOX_MULLER_ABS * gain[sl].max() / tol)
    return worst
