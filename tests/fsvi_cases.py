"""The case table of the FSVI step and the comparison both step tests share (a plain module).

pyz_fsvi_step launches k_fsvi_inputs, k_fsvi_stein_system, k_spd_solve_f64 (Stein), the Dense forward per layer with
per-particle input rows at layer 0, k_fsvi_gram, k_spd_solve_f64 (GP), k_fsvi_delta, k_dense_bwd_data / k_dense_bwd_weight
for the layers below the last, and k_fsvi_update.  This module restates which variant of each a case launches
(`expected_fsvi_launches`, on the rules of dense_cases), names the cells of the coverage table (`CELLS`, `reached_cells`),
lists the smallest cases that reach every cell, builds their inputs (`case_data`), restates one step in a chosen dtype on top
of fsvi_checks with the wrong variants the sensitivity check needs (`terms`, `MUTATIONS`, `standin_step`), and holds the
comparison of one step (`compare_step`).  tests/test_fsvi_dispatch_table.py pins all of it to the source and to
fsvi_checks.terms on the CPU; tests/test_gpu_fsvi_matrix.py runs the cases on the device.

Inputs whose Gram matrix is not I.  The length scale of the GP prior is 1, so rows drawn far apart give K_i = (1 + 1e-6) I
and alpha = f / (1 + 1e-6) whatever k_fsvi_gram computes off the diagonal.  Here the batch rows and the measurement rows of a
case are the n = b + B sites of one 2-D square lattice of spacing SPACING, dealt at random to the two sets, embedded in R^F by
a random orthonormal 2-frame, plus uniform jitter of +-`jitter` in every feature (fresh for the measurement rows of every
step), plus the injected noise z = 0.1 N(0, 1) of the step.  Every case, step and particle must then meet, from the Xp the
step itself assembled: COND_MIN <= cond(K_i) <= COND_MAX and a median over the rows of the largest off-diagonal entry of at
least ROWMAX_MIN (`input_conditions`).  The jitter is 0.2 except on `wide1`: there F = 300, the jitter's share of a squared
distance grows with F (300 x 2 x 0.2^2 / 3 = 8, a factor exp(-4) on every off-diagonal entry), and 0.2 sqrt(2 / F) keeps the
share of the 2-D cases.  Its spacing is 1.3: the measurement rows of particle i are shifted against its batch rows by z_0 +
... + z_(i-1), whose squared length grows with F too (300 x 0.01 = 3: a factor exp(-1.5) on every entry between the two
sets), and at spacing 1.6 particle 1 came out at cond 2.33, below the window; at 1.3 the two particles measure 13.5 and 4.1.
n = 514 needed no adjustment (the symbol of the lattice bounds cond by about 12 at any n: measured 12.5 to 13.1).  The figures
are printed by tests/test_fsvi_dispatch_table.py::test_input_conditions.

Targets are N(0, 1), and the last batch row of every step carries a target of magnitude EDGE: with b = 257 it is the one
loss row past 256, and a unit target could leave its residual too small for the loss bound to see it go.

Weights: mu = 0.3 N(0, 1), particles and every injected redraw mu + N(0, 1) 2 / sqrt(widest layer), so that the Stein system
K_w + 1e-3 I over the D weights stays below STEIN_COND_MAX.

A case takes two chained steps (t = 1, 2), each from the stored state of the one before, on other batch rows, measurement
rows and draws."""

from __future__ import annotations

import hashlib
from typing import NamedTuple, Optional

import numpy as np

import fsvi_checks as fc
from dense_cases import (LDS_MINWG, bwd_data_steps, bwd_data_tiles, cdiv, fwd_steps, fwd_takes_lds, fwd_tiles, lds_nt, pick_waves,
                         w_offsets, wgrad_steps, wgrad_tiles)
from head_cases import close_blocks
from oracle import mlp as o_mlp

F32 = np.float32

# ---------------------------------------------------------------- the rules (csrc/pyz_fsvi.h, pyz_api.hip pyz_fsvi_step)
STRIDE = 256               # threads of k_fsvi_gram, k_fsvi_stein_system, k_fsvi_delta, k_fsvi_inputs, k_fsvi_update
MAX_N, MAX_D = 1024, 2048  # PYZ_FSVI_MAX_N, PYZ_FSVI_MAX_D
SPD_MAX_N = 2048           # PYZ_SPD_MAX_N
SPD_LDS_N = 128            # PYZ_SPD_LDS_N
SPD_THREADS = 1024         # PYZ_SPD_THREADS
SPD_SMALL_N, SPD_SMALL_THREADS = 32, 256   # pyz_launch_spd: n <= 32 runs 256 threads


def spd_panel(n: int) -> int:
    """pyz_spd_panel"""
    return 32 if n <= 512 else (16 if n <= 1024 else 4)


def spd_threads(n: int) -> int:
    return SPD_SMALL_THREADS if n <= SPD_SMALL_N else SPD_THREADS


def spd_kernel(n: int) -> str:
    """pyz_launch_spd: the expression KernelProbe reports."""
    return "k_spd_solve_f64<true>" if n <= SPD_LDS_N else "k_spd_solve_f64<false>"


def spd_lds_bytes(n: int) -> int:
    """pyz_spd_lds_bytes"""
    if n <= SPD_LDS_N:
        return 8 * (3 * n + (n | 1) * n)
    return 8 * (2 * n + n * (spd_panel(n) + 1))


class FsviCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    k: int
    b: int                   # batch rows
    B: int                   # measurement rows (the batch_size hyper-parameter)
    gathered: bool = True    # the batch comes through row_idx (else rows 0 .. b - 1: the NULL arm)
    env: dict = {}           # PYZ_FWD_LDS_MINWG (read per call)
    jitter: float = 0.2
    spacing: float = 1.6

    @property
    def spec(self) -> o_mlp.MLPSpec:
        return o_mlp.MLPSpec(self.dims, self.acts, "mse")

    @property
    def D(self) -> int:
        return self.spec.n_params

    @property
    def F(self) -> int:
        return self.dims[0]

    @property
    def n(self) -> int:
        return self.b + self.B

    @property
    def L(self) -> int:
        return len(self.dims) - 1

    @property
    def H(self) -> int:
        """Inputs of the last layer: the H of k_fsvi_delta."""
        return self.dims[-2]

    @property
    def max_batch(self) -> int:
        return self.n + 3


class Fwd(NamedTuple):
    layer: int
    kernel: str
    S: int
    vec: int
    row_tiles: int
    col_tiles: int
    in_pstride: int


class Wg(NamedTuple):
    layer: int
    S: int
    tiles: int


class FsviLaunches(NamedTuple):
    gram_wgs: int            # workgroups of k_fsvi_gram per particle
    stein: str               # k_spd_solve_f64<LDS_A> of the Stein system, and its panel (0: in LDS)
    stein_panel: int
    gp: str
    gp_panel: int
    fwd: tuple
    bwd_data: tuple          # (layer, S)
    wgrad: tuple
    sequence: tuple          # the kernel expressions of a step in launch order, as KernelProbe reports them


def expected_fsvi_launches(case: FsviCase) -> FsviLaunches:
    """pyz_fsvi_step.  The forward is pyz_launch_fwd per layer on n = b + B rows and k particles, in_pstride = n F at layer 0
    (every particle its own rows: Xp is a fresh 16-byte aligned allocation) and max_batch K above; it does not go through the
    ring launcher.  k_fsvi_delta does the last layer's backward pass; launch_bwd_data_hidden gives delta[L - 3 .. 0];
    pyz_launch_bwd_weight runs for the layers L - 2 .. 0."""
    n, k, D, dims, L = case.n, case.k, case.D, case.dims, case.L
    offs = w_offsets(dims)
    min_wg = int(case.env.get("PYZ_FWD_LDS_MINWG", LDS_MINWG))
    fwd = []
    for l in range(L):
        K, N = dims[l], dims[l + 1]
        S, _ = pick_waves(fwd_tiles(n, N) * k, fwd_steps(K))
        in_ps = n * case.F if l == 0 else case.max_batch * K
        lds = fwd_takes_lds(K, N, n, k, D, offs[l], S, True, 1, min_wg) and (k == 1 or in_ps % 4 == 0)
        fwd.append(Fwd(l, f"k_dense_fwd_lds<{lds_nt(N)}>" if lds else "k_dense_fwd", S, int(K % 8 == 0), cdiv(n, 32), cdiv(N, 32), in_ps))
    bwd = tuple((l, pick_waves(bwd_data_tiles(n, dims[l]) * k, bwd_data_steps(dims[l + 1]))[0]) for l in range(L - 2, 0, -1))
    wg = tuple(Wg(l, pick_waves(wgrad_tiles(dims[l], dims[l + 1]) * k, wgrad_steps(n))[0], wgrad_tiles(dims[l], dims[l + 1]))
               for l in range(L - 2, -1, -1))
    stein, gp = spd_kernel(D), spd_kernel(n)
    seq = ("k_fsvi_inputs", "k_fsvi_stein_system", stein) + tuple(f.kernel for f in fwd) + ("k_fsvi_gram", gp, "k_fsvi_delta")
    seq += ("k_dense_bwd_data",) * len(bwd) + ("k_dense_bwd_weight",) * len(wg) + ("k_fsvi_update",)
    return FsviLaunches(cdiv(n * n, STRIDE), stein, 0 if D <= SPD_LDS_N else spd_panel(D), gp, 0 if n <= SPD_LDS_N else spd_panel(n),
                        tuple(fwd), bwd, wg, seq)


WATCHED = ("k_fsvi_", "k_spd_solve_f64", "k_dense_")


# ---------------------------------------------------------------- the coverage table
CELLS = frozenset([
    "gram: a second workgroup per particle", "gram: ragged last workgroup",
    "delta: a row r >= 256", "delta: a loss row r >= 256", "delta: ragged third trip of the row loop",
    "delta: j >= 256 in the last layer's loop", "delta: the bias j = H alone in the second trip",
    "delta: one-layer arm with F > 2", "delta: one-layer arm, second trip reads xp",
    "stein: second trip of the column loop", "stein: ragged last trip of the column loop",
    "gp solve in LDS", "gp solve n = 128 (last LDS size)", "gp solve n = 129 (first global size)",
    "gp solve global, panel 32", "gp solve global, panel 16",
    "stein solve in LDS", "stein solve global, panel 32", "stein solve global, panel 16", "stein solve global, panel 4",
    "layer 0 forward: more than one row tile", "layer 0 forward: more than one column tile", "layer 0 forward: vec = 1",
    "layer 0 forward: k_dense_fwd_lds on per-particle rows", "layer 0 forward: F = 4",
    "layer 0 weight gradient: more than one column tile", "layer 0 weight gradient: S > 1",
    "k_dense_bwd_data over k particles", "row_idx NULL", "row_idx gather", "b < B", "k = 3"])


def reached_cells(case: FsviCase) -> set:
    """The cells a case reaches, from its shape and `expected_fsvi_launches` alone."""
    la = expected_fsvi_launches(case)
    n, D, H, cells = case.n, case.D, case.H, set()
    if la.gram_wgs > 1:
        cells.add("gram: a second workgroup per particle")
    if (n * n) % STRIDE:
        cells.add("gram: ragged last workgroup")
    if n > STRIDE:
        cells.add("delta: a row r >= 256")
    if case.b > STRIDE:
        cells.add("delta: a loss row r >= 256")
    if n > 2 * STRIDE and n % STRIDE:
        cells.add("delta: ragged third trip of the row loop")
    if H >= STRIDE:
        cells.add("delta: j >= 256 in the last layer's loop")
    if H == STRIDE:
        cells.add("delta: the bias j = H alone in the second trip")
    if case.L == 1 and case.F > 2:
        cells.add("delta: one-layer arm with F > 2")
    if case.L == 1 and H > STRIDE:
        cells.add("delta: one-layer arm, second trip reads xp")
    if D > STRIDE:
        cells.add("stein: second trip of the column loop")
        if D % STRIDE:
            cells.add("stein: ragged last trip of the column loop")
    for sys_, size, panel in (("gp", n, la.gp_panel), ("stein", D, la.stein_panel)):
        cells.add(f"{sys_} solve in LDS" if panel == 0 else f"{sys_} solve global, panel {panel}")
    if n == SPD_LDS_N:
        cells.add("gp solve n = 128 (last LDS size)")
    if n == SPD_LDS_N + 1:
        cells.add("gp solve n = 129 (first global size)")
    if case.L > 1:
        f0 = la.fwd[0]
        if f0.row_tiles > 1:
            cells.add("layer 0 forward: more than one row tile")
        if f0.col_tiles > 1:
            cells.add("layer 0 forward: more than one column tile")
        if f0.kernel != "k_dense_fwd":
            cells.add("layer 0 forward: k_dense_fwd_lds on per-particle rows")
        elif f0.vec:
            cells.add("layer 0 forward: vec = 1")
        if case.F == 4:
            cells.add("layer 0 forward: F = 4")
        w0 = la.wgrad[-1]
        assert w0.layer == 0
        if cdiv(case.dims[1], 32) > 1:
            cells.add("layer 0 weight gradient: more than one column tile")
        if w0.S > 1:
            cells.add("layer 0 weight gradient: S > 1")
    if la.bwd_data and case.k > 1:
        cells.add("k_dense_bwd_data over k particles")
    cells.add("row_idx gather" if case.gathered else "row_idx NULL")
    if case.b < case.B:
        cells.add("b < B")
    if case.k == 3:
        cells.add("k = 3")
    return cells & CELLS


R, T, G, LN = "relu", "tanh", "sigmoid", "linear"
LDS_ANY = {"PYZ_FWD_LDS_MINWG": "1"}     # take k_dense_fwd_lds whenever the shape allows it


def _c(name, dims, acts, k, b, B, **kw):
    return FsviCase(name, tuple(dims), tuple(acts) + (LN,) if len(acts) < len(dims) - 1 else tuple(acts), k, b, B, **kw)


CASES = [
    _c("gram2", (2, 8, 1), (T,), 2, 8, 9),             # n = 17: two Gram workgroups, ragged; b < B
    _c("lds128", (2, 8, 1), (T,), 2, 64, 64),          # n = 128: GP solve at the last LDS size; 4 row tiles
    _c("glob129", (2, 8, 1), (T,), 2, 64, 65),         # n = 129: first global size, last panel of one column
    _c("rows514", (2, 8, 1), (T,), 2, 257, 257),       # third (ragged) trip of the delta loop, a loss row >= 256, GP panel 16
    _c("d161", (2, 40, 1), (R,), 3, 5, 5),             # Stein D = 161 global, panel 32; two column tiles
    _c("d385", (4, 64, 1), (T,), 2, 5, 5),             # Stein column loop second trip (ragged); F = 4
    _c("d601", (2, 150, 1), (G,), 2, 5, 5),            # Stein panel 16
    _c("h256", (2, 256, 1), (T,), 2, 5, 5),            # D = 1025: Stein panel 4; the bias j = H = 256 alone in the second trip
    _c("vec8", (8, 16, 1), (G,), 3, 3, 4, gathered=False),   # layer 0 vec = 1 with stride 56; the NULL gather
    _c("deep", (3, 40, 33, 1), (R, T), 2, 20, 20),     # D = 1547; k_dense_bwd_data over k particles, two row tiles
    _c("wide1", (300, 1), (LN,), 2, 5, 5, jitter=0.2 * float(np.sqrt(2.0 / 300.0)), spacing=1.3),   # one-layer arm, H = F = 300
    # an even D needs this odd-looking net: every two- and three-layer shape with an even first width has odd D and fails
    # the LDS kernel's theta_pstride % 2 rule
    _c("ldsfwd", (4, 64, 3, 2, 1), (T, T, T), 2, 64, 64, env=LDS_ANY),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"
N_STEPS = 2
LR = 0.05
SEED = 5          # the Philox seed of a call (unused by a step whose draws are all injected)

# ---------------------------------------------------------------- inputs
SPACING = 1.6
COND_MIN, COND_MAX, ROWMAX_MIN = 2.5, 100.0, 0.1
STEIN_COND_MAX = 1e7
EXTRA_ROWS = 3    # rows of x no batch uses (gathered: scattered among the others; else behind them)
FAR = 1.0e3       # what those rows hold
EDGE = 8.0        # magnitude of the target of the last batch row of a step


def lattice(n: int, spacing: float = SPACING) -> np.ndarray:
    """The first n sites, row by row, of a centred square lattice of spacing SPACING with ceil(sqrt(n)) columns."""
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    p = np.stack([i % side, i // side], axis=1).astype(np.float64)
    return spacing * (p - p.mean(axis=0))


def lattice_rows(n: int, F: int, rng, jitter: float = 0.2, spacing: float = SPACING):
    """(sites embedded in R^F by a random orthonormal 2-frame (n, F) float64, a function drawing their jittered rows)."""
    frame = np.linalg.qr(rng.normal(size=(F, 2)))[0]           # (F, 2), orthonormal columns
    emb = lattice(n, spacing) @ frame.T
    return emb, lambda sites: (emb[sites] + rng.uniform(-jitter, jitter, size=(len(sites), F))).astype(F32)


class Draws(NamedTuple):
    idx: Optional[np.ndarray]   # (b) int32 rows of x, or None
    xm: np.ndarray              # (B, F)
    z: np.ndarray               # (k, F)
    eps: np.ndarray             # (k, D)


class FsviData(NamedTuple):
    x: np.ndarray               # (b + EXTRA_ROWS, F)
    y: np.ndarray               # (b + EXTRA_ROWS, 1)
    mu0: np.ndarray
    W0: np.ndarray              # (k, D)
    steps: tuple                # Draws of step t = 1, 2


_DATA = {}


def case_data(case: FsviCase) -> FsviData:
    if case.name in _DATA:
        return _DATA[case.name]
    rng = np.random.default_rng(sum(map(ord, case.name)) + 7919)
    b, B, k, F, D, n = case.b, case.B, case.k, case.F, case.D, case.n
    _, rows_of = lattice_rows(n, F, rng, case.jitter, case.spacing)
    deal = rng.permutation(n)
    batch_sites, meas_sites = deal[:b], deal[b:]
    pos = rng.permutation(b + EXTRA_ROWS)[:b] if case.gathered else np.arange(b)
    x = np.full((b + EXTRA_ROWS, F), FAR, dtype=F32)
    x[pos] = rows_of(batch_sites)
    y = rng.normal(size=(b + EXTRA_ROWS, 1)).astype(F32)
    width = 2.0 / np.sqrt(max(case.dims))
    mu0 = (0.3 * rng.normal(size=D)).astype(F32)
    W0 = (mu0 + width * rng.normal(size=(k, D))).astype(F32)
    steps = []
    for _ in range(N_STEPS):
        idx = pos[rng.permutation(b)].astype(np.int32) if case.gathered else None
        last = int(idx[-1]) if case.gathered else b - 1
        y[last] = EDGE if y[last] >= 0 else -EDGE
        steps.append(Draws(idx, rows_of(meas_sites), (0.1 * rng.normal(size=(k, F))).astype(F32),
                           (width * rng.normal(size=(k, D))).astype(F32)))
    _DATA[case.name] = FsviData(x, y, mu0, W0, tuple(steps))
    return _DATA[case.name]


def batch_of(case: FsviCase, data: FsviData, d: Draws):
    rows = d.idx if d.idx is not None else np.arange(case.b)
    return data.x[rows], data.y[rows]


def initial_state(data: FsviData) -> dict:
    return {"mu": data.mu0.copy(), "m": np.zeros_like(data.mu0), "v": np.zeros_like(data.mu0), "W": data.W0.copy()}


def input_conditions(xp):
    """Per particle of Xp (k, n, F): (cond(K_i), median over the rows of the largest off-diagonal entry of K_i)."""
    out = []
    for xi in np.asarray(xp):
        K = fc.gram(xi)
        ev = np.linalg.eigvalsh(K)
        off = K - np.diag(np.diag(K))
        out.append((float(ev[-1] / ev[0]), float(np.median(off.max(axis=1)))))
    return out


def assert_input_conditions(xp, what=""):
    conds = input_conditions(xp)
    for i, (cond, med) in enumerate(conds):
        assert COND_MIN <= cond <= COND_MAX, f"{what}: particle {i}: cond(K_i) = {cond:.3g} outside [{COND_MIN}, {COND_MAX}]"
        assert med >= ROWMAX_MIN, f"{what}: particle {i}: median row maximum off the diagonal {med:.3g} < {ROWMAX_MIN}"
    return conds


def stein_cond(w) -> float:
    ev = np.linalg.eigvalsh(fc.stein_system(w)[0])
    return float(ev[-1] / ev[0])


# ---------------------------------------------------------------- one step, restated (any dtype, wrong variants)
M_GRAM = ("Gram distance without the last feature", "Gram with exp(-d^2) in place of exp(-d^2 / 2)", "Gram off-diagonal zeroed",
          "Gram jitter missing")
M_DELTA = ("delta rows >= 256 dropped", "loss rows >= 256 dropped", "last layer's bias gradient missing at H >= 256")
M_STEIN = ("Stein columns >= 256 dropped", "Stein rhs without 1 / D", "c2 with the wrong sign")
M_INPUT = ("layer 0's forward fed with particle 0's rows", "layer 0's weight gradient fed with particle 0's rows",
           "measurement rows shifted by z_i alone")
M_SCALE = ("k / B read as 1 / (B k)",)
MUTATIONS = M_GRAM + M_DELTA + M_STEIN + M_INPUT + M_SCALE


def mutation_applies(case: FsviCase, mutation: str) -> bool:
    if mutation == M_DELTA[0]:
        return case.n > STRIDE
    if mutation == M_DELTA[1]:
        return case.b > STRIDE
    if mutation == M_DELTA[2]:
        return case.H >= STRIDE
    if mutation == M_STEIN[0]:
        return case.D > STRIDE
    if mutation == M_INPUT[1]:
        return case.k > 1 and case.L > 1     # (a one-layer model's only weight gradient is k_fsvi_delta's)
    if mutation in M_INPUT or mutation in M_SCALE:
        return case.k > 1
    return True


def _gram(xp_i, mutation=None):
    x = np.asarray(xp_i, np.float64)
    if mutation == M_GRAM[0]:
        x = x[:, :-1]
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    K = np.exp(-d2 if mutation == M_GRAM[1] else -0.5 * d2)
    if mutation == M_GRAM[2]:
        K = np.eye(len(x))
    return K if mutation == M_GRAM[3] else K + fc.JITTER * np.eye(len(x))


_C2 = {}


def _stein_c2(w, mutation=None):
    """fc.stein_c2 and its wrong variants, rounded to float32 once; kept per weight vector (D up to 1547)."""
    w = np.asarray(w, F32)
    mutation = mutation if mutation in M_STEIN else None
    key = (hashlib.sha1(w.tobytes()).hexdigest(), mutation)
    if key not in _C2:
        if mutation is None:
            c2 = fc.stein_c2(w)
        else:
            w64 = w.astype(np.float64)
            diff = w64[:, None] - w64[None, :]
            K = np.exp(-0.5 * diff * diff)
            terms_ = -diff * K
            if mutation == M_STEIN[0]:
                terms_ = terms_[:, :STRIDE]
            rhs = terms_.sum(axis=1) / (1.0 if mutation == M_STEIN[1] else len(w))
            c2 = np.linalg.solve(K + fc.REG * np.eye(len(w)), rhs)
            c2 = c2 if mutation == M_STEIN[2] else -c2
        if len(_C2) > 64:
            _C2.clear()
        _C2[key] = c2.astype(F32).astype(np.float64)
    return _C2[key]


def _backprop(theta, acts, delta_out, spec, dt, x_wgrad=None):
    """fc.backprop on the activations of a forward pass in dt; x_wgrad: other rows under layer 0's weight gradient."""
    ws = o_mlp.unpack(np.asarray(theta, dtype=dt), spec)
    delta = np.asarray(delta_out, dtype=dt).reshape(-1, 1) * o_mlp._act_grad_from_output(acts[-1], spec.acts[-1])
    grads = [None] * spec.n_layers
    for l in range(spec.n_layers - 1, -1, -1):
        a = acts[l] if (l > 0 or x_wgrad is None) else np.asarray(x_wgrad, dtype=dt)
        grads[l] = (a.T @ delta, delta.sum(axis=0))
        if l > 0:
            delta = (delta @ ws[l][0].T) * o_mlp._act_grad_from_output(acts[l], spec.acts[l - 1])
    return o_mlp.pack(grads)


def terms(case: FsviCase, W, xd, y, xm, z, dtype=np.float64, mutation=None) -> dict:
    """fsvi_checks.terms (steps 2-7 and 9 of A8) with the forward pass, the delta and the backward pass in `dtype`, the two
    solves in float64 on the float32 weights and on f as `dtype` left it, and `mutation` one of the wrong variants above.
    float64 and no mutation: fc.terms itself (tests/test_fsvi_dispatch_table.py holds the two together)."""
    dt, spec, B = dtype, case.spec, case.B
    W = np.asarray(W, F32)
    k, b = len(W), len(xd)
    yv = np.asarray(y, dt).reshape(-1)
    scale = 1.0 / (B * k) if mutation == M_SCALE[0] else k / B
    xp = fc.make_xp(xd, xm, z, "fresh" if mutation == M_INPUT[2] else "prefix")
    f_all, alpha_all, c2_all = [], [], []
    g = np.zeros(W.shape[1], dtype=dt)
    c2_sum = np.zeros(W.shape[1], dtype=dt)
    loss = 0.0
    for i in range(k):
        acts, _ = o_mlp.forward(W[i], xp[0] if mutation == M_INPUT[0] else xp[i], spec, dt)
        f = acts[-1].reshape(-1)
        alpha = np.linalg.solve(_gram(xp[i], mutation), f.astype(np.float64))
        c2 = _stein_c2(W[i], mutation)
        e = f[:b] - yv
        delta = (-alpha / k).astype(dt)
        delta[:b] += (dt(scale * (2.0 / b)) * e).astype(dt)
        if mutation == M_DELTA[0]:
            delta[STRIDE:] = 0
        gi = _backprop(W[i], acts, delta, spec, dt, xp[0] if mutation == M_INPUT[1] else None)
        if mutation == M_DELTA[2]:
            gi[spec.offsets()[-1][1]:] = 0
        g += gi
        c2_sum += c2.astype(dt)
        e64 = e.astype(np.float64)
        if mutation == M_DELTA[1]:
            loss += (e64[:STRIDE] ** 2).sum() / b / k
        else:
            loss += (e64 ** 2).mean() / k
        f_all.append(f)
        alpha_all.append(alpha)
        c2_all.append(c2)
    g = g - c2_sum / dt(k)
    return dict(xp=xp, f=np.stack(f_all), alpha=np.stack(alpha_all), c2=np.stack(c2_all), g=g, loss=loss)


def ref_step(case: FsviCase, data: FsviData, t: int, s0: dict) -> dict:
    """The float64 reference of step t from the stored state s0."""
    d = data.steps[t - 1]
    xd, y = batch_of(case, data, d)
    return terms(case, s0["W"], xd, y, d.xm, d.z)


def standin_step(case: FsviCase, data: FsviData, t: int, s0: dict, mutation=None) -> dict:
    """What a float32 device would leave of step t: terms in float32, k_fsvi_update's float32 Adam on its own g, the redraw."""
    d = data.steps[t - 1]
    xd, y = batch_of(case, data, d)
    out = terms(case, s0["W"], xd, y, d.xm, d.z, F32, mutation)
    g = out["g"].astype(F32)
    mu, m, v = fc.adam32(s0["mu"], g, s0["m"], s0["v"], t, LR)
    return dict(xp=out["xp"], f=out["f"].astype(F32), alpha=out["alpha"], c2=out["c2"].astype(F32), g=g,
                loss=np.array([out["loss"]], dtype=F32), mu=mu.astype(F32), m=m.astype(F32), v=v.astype(F32),
                W=(mu.astype(F32)[None, :] + d.eps).astype(F32))


def stored(got: dict) -> dict:
    return {q: got[q] for q in ("mu", "m", "v", "W")}


# ---------------------------------------------------------------- the comparison of one step
REL_G, REL_LOSS, REL_F, REL_ALPHA, REL_C2, REL_ADAM = 1e-4, 1e-4, 1e-4, 1e-9, 1e-6, 1e-6   # DESIGN 8, tests/test_gpu_fsvi.py


def _close(got, ref, rel, what) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite entries"
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max()
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e} > {rel:g})"
    return float(err / (rel * scale))


def compare_step(case: FsviCase, data: FsviData, t: int, s0: dict, got: dict, ref: Optional[dict] = None, what: str = "") -> dict:
    """One step's result `got` (a device's, or a stand-in's) from the stored state s0 against the float64 reference `ref`
    (computed when not given).  Raises AssertionError on the first bound missed; returns quantity -> error over tolerance.

    xp, W:   bit for bit (make_xp; mu + eps, one float32 add)
    alpha:   per particle at 1e-9 against NumPy's solve of the restated K_i on got's own f
    c2:      per particle at 1e-6
    f:       at 1e-4
    g:       per layer block (W_l, b_l) at 1e-4 of the block's largest magnitude, floor 1e-3 of the largest over all blocks
    loss:    at 1e-4
    mu, m, v: at 1e-6 against fsvi_checks.adam32 on got's own g"""
    what = f"{what}{case.name} t={t}"
    d = data.steps[t - 1]
    ref = ref if ref is not None else ref_step(case, data, t, s0)
    rep = {}
    assert np.array_equal(np.asarray(got["xp"], F32).view(np.int32), ref["xp"].view(np.int32)), f"{what}: xp differs from make_xp"
    f = np.asarray(got["f"], np.float64)
    rep["alpha"] = max(_close(got["alpha"][i], fc.gp_alpha(fc.gram(ref["xp"][i]), f[i]), REL_ALPHA, f"{what}: alpha of particle {i}")
                       for i in range(case.k))
    rep["c2"] = max(_close(got["c2"][i], ref["c2"][i], REL_C2, f"{what}: c2 of particle {i}") for i in range(case.k))
    rep["f"] = _close(f, ref["f"], REL_F, f"{what}: f")
    rep["g"] = close_blocks(got["g"], ref["g"], case.spec, REL_G, f"{what}: g")
    rep["loss"] = _close(np.asarray(got["loss"]).reshape(-1), [ref["loss"]], REL_LOSS, f"{what}: loss")
    mu1, m1, v1 = fc.adam32(s0["mu"], got["g"], s0["m"], s0["v"], t, LR)
    for q, r in (("mu", mu1), ("m", m1), ("v", v1)):
        rep[q] = _close(got[q], r, REL_ADAM, f"{what}: {q}")
    want = (np.asarray(got["mu"], F32)[None, :] + d.eps).astype(F32)
    assert np.array_equal(np.asarray(got["W"], F32).view(np.int32), want.view(np.int32)), f"{what}: the redraw is not mu + eps"
    return rep
