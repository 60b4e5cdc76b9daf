"""The Deep-PILCO rollout kernels (csrc/pyz_pilco.h) as an accounting of paths: a case table with per-layer policy
layers and per-layer dynamics activations, a plain-Python restatement of the host rules that decide which loop trips
and which branch arms a shape reaches, the named cells those rules give, and deliberately wrong oracles.  Nothing here
touches the library under test; the float64 oracle is pilco_rbf_checks.rollout, unchanged.

A cell is one arm of a branch or one trip count of a loop.  CELLS = OLD_CELLS | NEW_CELLS: OLD_CELLS are what the sixteen
cases of pilco_checks / pilco_rbf_checks reach, NEW_CELLS what only the cases of this table reach.  ROW_OWNER names, for
every path the sixteen never took, the case that was made for it; OWNED[name] is a cell that `name` alone reaches.
tests/test_pilco_dispatch_table.py pins the restatement to the source and the cells to the cases;
tests/test_gpu_pilco_matrix.py runs the cases.

Inputs are drawn as pilco_checks.make_inputs draws them (Dense kernels N(0, gain^2 / fan_in), gain 1 for the policy and
0.7 for the dynamics, biases N(0, 0.1^2), RBF means N(0, 0.5^2), s0 uniform in +-0.05, eps unit normals) from
numpy.random.default_rng([seed, 77]), seed 3 unless SEED says otherwise."""

from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np
import torch

import pilco_checks as pc
import pilco_rbf_checks as rc

GAMMA = pc.GAMMA
TOL = 1e-4                      # the GPU bound of test_gpu_pilco*.py, unchanged: of max |ref|; the cost relative

# ---------------------------------------------------------------- the constants of pyz_pilco.h
MAX_LAYERS, MAX_WIDTH, MAX_K, MAX_IN, MAX_H, THREADS = 8, 512, 256, 64, 4096, 256
GRAPH_SLOTS = 4                 # PyzGraphCache<4>, keyed by (H, freq)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    name: str
    S: int
    A: int
    K: int
    H: int
    pol_hidden: Tuple[tuple, ...]       # ("dense", units, activation) | ("rbf", units, gamma)
    pol_out: str
    dyn_hidden: Tuple[tuple, ...]       # (units, activation)
    reward: str
    freq: Optional[int] = None          # None: default_freq(H)
    also_freq: Tuple[int, ...] = ()     # further rollouts of the same plan and inputs
    max_horizon: Optional[int] = None   # of the plan; None: H

    @property
    def pol_dims(self):
        return (self.S,) + tuple(l[1] for l in self.pol_hidden) + (self.A,)

    @property
    def pol_kinds(self):
        return tuple(l[0] for l in self.pol_hidden) + ("dense",)

    @property
    def pol_acts(self):
        return tuple("linear" if l[0] == "rbf" else l[2] for l in self.pol_hidden) + (self.pol_out,)

    @property
    def pol_gammas(self):
        return tuple(float(l[2]) if l[0] == "rbf" else 0.0 for l in self.pol_hidden) + (0.0,)

    @property
    def dyn_dims(self):
        return (self.S + self.A,) + tuple(l[0] for l in self.dyn_hidden) + (self.S,)

    @property
    def dyn_acts(self):
        return tuple(l[1] for l in self.dyn_hidden) + ("linear",)

    @property
    def freqs(self):
        return (pc.default_freq(self.H) if self.freq is None else self.freq,) + self.also_freq

    @property
    def plan_horizon(self):
        return self.H if self.max_horizon is None else self.max_horizon


def _dense(*units, act="tanh"):
    return tuple(("dense", u, act) for u in units)


_MIX = ("tanh", "sigmoid", "relu", "tanh", "relu", "sigmoid", "tanh")      # deep8: the activation of hidden layer l
H_GRID = 600
# The smallest shapes that reach each cell.  Two figures are not the first ones thought of:
# h257 at its default freq 10 and at 7 counts no step past 252: the second trip of k_pilco_close's cost loop would add
# zeros only, and at freq 1 steps 256 and 257 weigh 0.95^256 = 2e-6.  freq 128 counts step 256 at 0.95^2.
# h_grid has K = 3, not 2: with two particles sd = |y_1 - y_2| / 2, and over 600 steps x 4 columns it comes within 1e-3 of
# zero for every seed tried (the best of forty: 5e-4).  K has no part in the grid rule the case is for.
NEW_CASES = [
    Case("ks258", 6, 3, 43, 3, _dense(8), "softmax", ((16, "tanh"),), "Acb 2 factors"),
    Case("kmax_in64", 63, 1, 256, 2, _dense(8), "tanh", ((16, "tanh"),), "Cart"),
    Case("wide_softmax", 40, 24, 4, 3, _dense(12), "softmax", ((20, "tanh"),), "Acb 2 factors"),
    Case("pol_257", 6, 3, 3, 4, _dense(257), "softmax", ((16, "tanh"),), "Acb 2 factors"),
    Case("b128_129", 4, 2, 5, 6, _dense(129, 128), "softmax", ((128, "tanh"), (129, "tanh")), "Cart"),
    Case("b256_257", 4, 2, 3, 3, _dense(256, 257), "softmax", ((257, "tanh"), (256, "tanh")), "Cart"),
    Case("w512", 5, 2, 3, 3, _dense(512, 512), "softmax", ((512, "tanh"),), "Acb 2 factors"),
    Case("deep8", 4, 2, 3, 3, tuple(("dense", 9 + l, _MIX[l]) for l in range(7)), "sigmoid",
         tuple((9 + l, _MIX[(l + 3) % 7]) for l in range(7)), "Cart"),
    Case("dense_then_rbf_wide", 4, 2, 5, 4, (("dense", 257, "tanh"), ("rbf", 17, 1.0 / 257)), "softmax", ((16, "tanh"),), "Cart"),
    Case("h257", 4, 2, 3, 257, _dense(8), "softmax", ((16, "tanh"),), "Cart", also_freq=(7, 128), max_horizon=4096),
    Case("h_grid", 4, 1, 3, H_GRID, (), "linear", (), "Cart"),
    Case("tail_uncounted", 5, 4, 9, 5, _dense(8), "sigmoid", ((16, "tanh"),), "Acb 2 factors", freq=2, also_freq=(6,)),
]
NEW = tuple(c.name for c in NEW_CASES)
OLD = tuple(c.name for c in pc.CASES) + tuple(c.name for c in rc.CASES)
CASE = {c.name: c for c in NEW_CASES}
SEED = {}                                   # name -> seed, should 3 leave a relu pre-activation of a case on its kink (none does)
# the graph-cache test of test_gpu_pilco_matrix.py: h257's nets on a plan of 64 steps, five (H, freq) pairs
GRAPH_PAIRS = ((8, 1), (9, 1), (10, 2), (11, 3), (12, 5))
DEDICATED = {"graph_cache": ("graph cache: fifth (H, freq) pair evicts the least recently used slot",
                             "graph cache: a changed pointer drops every slot (rekey)")}


def view(name):
    """What the rules read of a case of any of the three tables."""
    if name in CASE:
        c = CASE[name]
        return SimpleNamespace(name=name, S=c.S, A=c.A, K=c.K, H=c.H, pol_dims=c.pol_dims, pol_kinds=c.pol_kinds,
                               pol_acts=c.pol_acts, dyn_dims=c.dyn_dims, dyn_acts=c.dyn_acts, reward=c.reward,
                               freqs=c.freqs, plan_horizon=c.plan_horizon)
    c = pc.CASE[name] if name in pc.CASE else rc.CASE[name]
    kinds = getattr(c, "pol_kinds", ("dense",) * len(c.pol_acts))
    return SimpleNamespace(name=name, S=c.S, A=c.A, K=c.K, H=c.H, pol_dims=c.pol_dims, pol_kinds=kinds, pol_acts=c.pol_acts,
                           dyn_dims=c.dyn_dims, dyn_acts=c.dyn_acts, reward=c.reward, freqs=(c.freq,), plan_horizon=c.H)


# ---------------------------------------------------------------- the host rules, restated
def pilco_fwd_lds(K, S, maxw):
    return 4 * (K * S + MAX_IN + 2 * maxw + THREADS)


def pilco_act_lds(maxw):
    return 4 * (MAX_IN + 2 * maxw + THREADS)


def pilco_bwd_lds(K, S, maxw, pw):
    return 4 * (2 * K * S + MAX_IN + pw + 2 * maxw + THREADS)


def n_params(dims, kinds=None):
    kinds = kinds or ("dense",) * (len(dims) - 1)
    return sum(i * o if k == "rbf" else (i + 1) * o for i, o, k in zip(dims[:-1], dims[1:], kinds))


def host_plan(K, pol_dims, dyn_dims, pol_kinds=None):
    """pyz_pilco_create_layers: maxw, tw_pol, tw, pw, Dp, Dd, the LDS of the three kernels and the branch taken on it."""
    S, A = pol_dims[0], pol_dims[-1]
    maxw = max((MAX_IN,) + tuple(pol_dims) + tuple(dyn_dims))
    tw_pol = sum(pol_dims[1:-1])
    tw = tw_pol + sum(dyn_dims[1:-1])
    pw = S + tw_pol + A
    fwd, bwd = pilco_fwd_lds(K, S, maxw), pilco_bwd_lds(K, S, maxw, pw)
    lds = max(fwd, bwd)
    branch = "refused" if lds > 160 * 1024 else "attribute" if lds > 64 * 1024 else "plain"
    return SimpleNamespace(S=S, A=A, K=K, maxw=maxw, tw_pol=tw_pol, tw=tw, pw=pw, Dp=n_params(pol_dims, pol_kinds),
                           Dd=n_params(dyn_dims), fwd_lds=fwd, bwd_lds=bwd, act_lds=pilco_act_lds(maxw), lds=lds, branch=branch)


def tiles(dims):
    return sum(cdiv(i, 32) * cdiv(o, 32) for i, o in zip(dims[:-1], dims[1:]))


def set_grid(K, pol_dims, dyn_dims, H):
    """The grid of k_pilco_set and what decided its width."""
    t, h = max(tiles(pol_dims), tiles(dyn_dims)), cdiv(H + 1, 256)
    return (max(t, h), K + 2), ("H" if h > t else "tiles")


def admissible(K, pol_dims, dyn_dims, max_horizon, pol_acts=None):
    """The limits pyz_pilco_create_layers checks before it looks for a device (None, or what is refused)."""
    S, A = pol_dims[0], pol_dims[-1]
    for what, dims in (("policy", pol_dims), ("dynamics", dyn_dims)):
        if not 1 <= len(dims) - 1 <= MAX_LAYERS:
            return f"{what}: layers"
        if any(not 1 <= d <= MAX_WIDTH for d in dims):
            return f"{what}: width"
    if pol_acts and "softmax" in pol_acts[:-1]:
        return "policy: softmax on a hidden layer"
    if not 2 <= K <= MAX_K:
        return "particles"
    if not 1 <= max_horizon <= MAX_H:
        return "max_horizon"
    if S + A > MAX_IN:
        return "S + A"
    if dyn_dims[0] != S + A or dyn_dims[-1] != S:
        return "dynamics dims"
    return None


def coef(t, H, freq, gamma, K):
    """c_t of k_pilco_set."""
    if t == 0:
        return -1.0 / K
    return -gamma ** (t // freq) / K if t % freq == 0 else 0.0


def choice(red, out):
    """The per-layer choice of pilco_gemv / pilco_rbf (red = Kin, out = N) and, with the roles swapped, of the transposed
    back-propagation and of pilco_rbf_dx (red = N, out = Kin): `out` values, each a sum over `red` terms."""
    if out > THREADS // 2:
        trips = cdiv(out, THREADS)
        return SimpleNamespace(path="wide", trips=trips, clamped=trips * THREADS - out, NP=None, G=None, len=None, padded=0,
                               empty=0)
    NP = 1
    while NP < out:
        NP <<= 1
    G = THREADS // NP
    ln = cdiv(red, G)
    ranges = [(min(g * ln, red), min(min(g * ln, red) + ln, red)) for g in range(G)]
    assert sum(b - a for a, b in ranges) == red
    return SimpleNamespace(path="split", trips=1, clamped=0, NP=NP, G=G, len=ln, padded=NP - out,
                           empty=sum(1 for a, b in ranges if a == b))


USES = ("policy forward", "dynamics forward", "dynamics backward", "policy backward")


def layer_choices(v):
    """[(use, function, layer, choice)] for the four uses of the per-layer choice."""
    out = []
    for l, (i, o, k) in enumerate(zip(v.pol_dims[:-1], v.pol_dims[1:], v.pol_kinds)):
        out.append(("policy forward", "pilco_rbf" if k == "rbf" else "pilco_gemv", l, choice(i, o)))
        out.append(("policy backward", "pilco_rbf_dx" if k == "rbf" else "pilco_gemv", l, choice(o, i)))
    for l, (i, o) in enumerate(zip(v.dyn_dims[:-1], v.dyn_dims[1:])):
        out.append(("dynamics forward", "pilco_gemv", l, choice(i, o)))
        out.append(("dynamics backward", "pilco_gemv", l, choice(o, i)))
    return out


def _choice_cells(use, fn, c):
    if c.path == "wide":
        return [f"{use}, {fn}: wide path, {c.trips} trip{'s' if c.trips > 1 else ''}, "
                f"{'clamped lanes' if c.clamped else 'no clamped lane'}"]
    cells = [f"{use}, {fn}: split path, NP {'>' if c.padded else '=='} N"]
    if c.G == 2:
        cells.append(f"{use}, {fn}: split path, G == 2")
    if c.empty:
        cells.append(f"{use}, {fn}: split path, empty groups")
    return cells


def reached_cells(name):
    """The cells a case (or a dedicated test) reaches, from the restatement alone."""
    if name in DEDICATED:
        return set(DEDICATED[name])
    v = view(name)
    p = host_plan(v.K, v.pol_dims, v.dyn_dims, v.pol_kinds)
    cells = set()
    for use, fn, _, c in layer_choices(v):
        cells.update(_choice_cells(use, fn, c))
    KS = v.K * v.S
    cells.add("staging: K S <= 256, one trip" if KS <= 256 else
              "staging: ragged second trip" if KS < 512 and KS % 256 else "staging: many whole trips")
    rbf = "rbf" in v.pol_kinds
    cells.add("pact: pw <= 256" if p.pw <= 256 else f"pact: pw > 256, {'an RBF' if rbf else 'a Dense-only'} policy")
    # the policy's shape
    Lp, Ld = len(v.pol_dims) - 1, len(v.dyn_dims) - 1
    hidden = v.pol_kinds[:-1]
    cells.add("policy: no hidden layer" if Lp == 1 else "policy: one hidden layer" if Lp == 2 else "policy: two or more hidden layers")
    for a, b in zip(hidden[:-1], hidden[1:]):
        cells.add(f"policy: {a} then {b} hidden layers")
    if Lp == 2 and hidden == ("dense",) and v.pol_dims[1] > THREADS:
        cells.add("policy: one Dense hidden layer of more than 256 units")
    if Lp == MAX_LAYERS:
        cells.add("policy: L == 8")
    if Ld == MAX_LAYERS:
        cells.add("dynamics: L == 8")
    cells.add("dynamics: no hidden layer" if Ld == 1 else "dynamics: hidden layers")
    if len({a for a, k in zip(v.pol_acts[:-1], hidden) if k == "dense"}) > 1 or len(set(v.dyn_acts[:-1])) > 1:
        cells.add("activations differ from layer to layer")
    if max(v.pol_dims) == MAX_WIDTH:
        cells.add("policy: a layer of PILCO_MAX_WIDTH")
    cells.add(f"policy output: {v.pol_acts[-1]}")
    if v.pol_acts[-1] == "softmax":
        cells.add("softmax: A <= 3" if v.A <= 3 else "softmax: A > 3")
    if v.S + v.A == MAX_IN:
        cells.add("S + A == 64")
        if v.A > 1:
            cells.add("S + A == 64 with A > 1")
    if v.K == MAX_K:
        cells.add("K == 256")
    if v.K % 8:
        cells.add("K % 8 != 0")
    if v.reward == "Acb 2 factors" and v.S == 5:
        cells.add("Acb at S == 5")
    cells.add(f"LDS: {p.branch}")
    for freq in v.freqs:
        counted = [t for t in range(1, v.H + 1) if coef(t, v.H, freq, GAMMA, v.K) != 0.0]
        cells.add("tail: nothing counted (freq > H)" if not counted else
                  "tail: c_H != 0" if counted[-1] == v.H else "tail: c_H == 0 (H % freq != 0)")
    trips = cdiv(v.H + 1, 256)
    cells.add("close: cost loop, one trip" if trips == 1 else "close: cost loop, two trips" if trips == 2 else
              "close: cost loop, three trips or more")
    if v.H >= 256:
        cells.add("set: coefficient row with t >= 256")
    cells.add(f"set: grid width from {set_grid(v.K, v.pol_dims, v.dyn_dims, v.H)[1]}")
    if v.plan_horizon == MAX_H:
        cells.add("plan: max_horizon == 4096")
    return cells


# what the sixteen cases of pilco_checks / pilco_rbf_checks reach (test_pilco_dispatch_table.py: exactly this set)
OLD_CELLS = frozenset("""
K % 8 != 0
LDS: plain
close: cost loop, one trip
dynamics backward, pilco_gemv: split path, G == 2
dynamics backward, pilco_gemv: split path, NP == N
dynamics backward, pilco_gemv: split path, NP > N
dynamics backward, pilco_gemv: split path, empty groups
dynamics backward, pilco_gemv: wide path, 1 trip, no clamped lane
dynamics backward, pilco_gemv: wide path, 2 trips, no clamped lane
dynamics forward, pilco_gemv: split path, G == 2
dynamics forward, pilco_gemv: split path, NP == N
dynamics forward, pilco_gemv: split path, NP > N
dynamics forward, pilco_gemv: split path, empty groups
dynamics forward, pilco_gemv: wide path, 1 trip, no clamped lane
dynamics forward, pilco_gemv: wide path, 2 trips, no clamped lane
dynamics: hidden layers
pact: pw <= 256
pact: pw > 256, an RBF policy
policy backward, pilco_gemv: split path, G == 2
policy backward, pilco_gemv: split path, NP == N
policy backward, pilco_gemv: split path, NP > N
policy backward, pilco_gemv: split path, empty groups
policy backward, pilco_gemv: wide path, 2 trips, clamped lanes
policy backward, pilco_rbf_dx: split path, NP == N
policy backward, pilco_rbf_dx: split path, NP > N
policy backward, pilco_rbf_dx: split path, empty groups
policy forward, pilco_gemv: split path, G == 2
policy forward, pilco_gemv: split path, NP == N
policy forward, pilco_gemv: split path, NP > N
policy forward, pilco_gemv: split path, empty groups
policy forward, pilco_rbf: split path, G == 2
policy forward, pilco_rbf: split path, NP == N
policy forward, pilco_rbf: split path, NP > N
policy forward, pilco_rbf: split path, empty groups
policy forward, pilco_rbf: wide path, 2 trips, clamped lanes
policy output: linear
policy output: relu
policy output: softmax
policy: dense then rbf hidden layers
policy: no hidden layer
policy: one hidden layer
policy: rbf then dense hidden layers
policy: two or more hidden layers
set: grid width from tiles
softmax: A <= 3
staging: K S <= 256, one trip
tail: c_H != 0
""".strip().splitlines())

# the paths the sixteen never took -> the case made for each (it reaches the cell; it need not be the only one)
ROW_OWNER = {
    "staging: ragged second trip": "ks258",
    "staging: many whole trips": "kmax_in64",
    "policy forward, pilco_gemv: wide path, 1 trip, clamped lanes": "b128_129",
    "policy forward, pilco_gemv: wide path, 1 trip, no clamped lane": "b256_257",
    "policy forward, pilco_gemv: wide path, 2 trips, clamped lanes": "pol_257",
    "policy forward, pilco_gemv: wide path, 2 trips, no clamped lane": "w512",
    "policy backward, pilco_gemv: wide path, 1 trip, clamped lanes": "b128_129",
    "policy backward, pilco_gemv: wide path, 1 trip, no clamped lane": "b256_257",
    "policy backward, pilco_gemv: wide path, 2 trips, no clamped lane": "w512",
    "dynamics forward, pilco_gemv: wide path, 1 trip, clamped lanes": "b128_129",
    "dynamics forward, pilco_gemv: wide path, 2 trips, clamped lanes": "b256_257",
    "dynamics backward, pilco_gemv: wide path, 1 trip, clamped lanes": "b128_129",
    "dynamics backward, pilco_gemv: wide path, 2 trips, clamped lanes": "b256_257",
    "pact: pw > 256, a Dense-only policy": "pol_257",
    "policy: one Dense hidden layer of more than 256 units": "pol_257",
    "policy backward, pilco_rbf_dx: wide path, 2 trips, clamped lanes": "dense_then_rbf_wide",
    "policy: dense then dense hidden layers": "b128_129",
    "policy: L == 8": "deep8",
    "dynamics: L == 8": "deep8",
    "activations differ from layer to layer": "deep8",
    "policy: a layer of PILCO_MAX_WIDTH": "w512",
    "Acb at S == 5": "w512",
    "policy output: tanh": "kmax_in64",
    "policy output: sigmoid": "deep8",
    "softmax: A > 3": "wide_softmax",
    "S + A == 64": "kmax_in64",
    "S + A == 64 with A > 1": "wide_softmax",
    "K == 256": "kmax_in64",
    "LDS: attribute": "kmax_in64",
    "tail: c_H == 0 (H % freq != 0)": "tail_uncounted",
    "tail: nothing counted (freq > H)": "tail_uncounted",
    "close: cost loop, two trips": "h257",
    "close: cost loop, three trips or more": "h_grid",
    "set: coefficient row with t >= 256": "h257",
    "set: grid width from H": "h_grid",
    "plan: max_horizon == 4096": "h257",
    "dynamics: no hidden layer": "h_grid",
    "graph cache: fifth (H, freq) pair evicts the least recently used slot": "graph_cache",
    "graph cache: a changed pointer drops every slot (rekey)": "graph_cache",
}
NEW_CELLS = frozenset(ROW_OWNER)
CELLS = OLD_CELLS | NEW_CELLS
# a cell that the case alone reaches: dropping the case loses it
OWNED = {
    "ks258": "staging: ragged second trip",
    "kmax_in64": "LDS: attribute",
    "wide_softmax": "softmax: A > 3",
    "pol_257": "policy: one Dense hidden layer of more than 256 units",
    "b128_129": "policy forward, pilco_gemv: wide path, 1 trip, clamped lanes",
    "b256_257": "policy forward, pilco_gemv: wide path, 1 trip, no clamped lane",
    "w512": "policy: a layer of PILCO_MAX_WIDTH",
    "deep8": "policy: L == 8",
    "dense_then_rbf_wide": "policy backward, pilco_rbf_dx: wide path, 2 trips, clamped lanes",
    "h257": "close: cost loop, two trips",
    "h_grid": "set: grid width from H",
    "tail_uncounted": "tail: nothing counted (freq > H)",
    "graph_cache": "graph cache: fifth (H, freq) pair evicts the least recently used slot",
}
# The one refusal no admissible shape reaches: `lds > 160 KB` in pyz_pilco_create_layers.  The largest plan the other
# limits admit is K = 256, S = 63, A = 1 with seven 512-wide policy hidden layers: 148 992 bytes (max_admissible_lds).
UNREACHABLE = "LDS: refused"


def max_admissible_lds():
    """(bytes, K, pol_dims, dyn_dims) of the largest LDS over the corners of what `admissible` admits.  The LDS grows with
    K, with S (K S), with every width (maxw, pw) and with the policy's depth (pw), and S + A <= 64 trades S against A, so
    the maximum sits at K = 256, widths 512, L = 8 and some split of 64 into S and A: every split is tried."""
    best = None
    for S in range(1, MAX_IN):
        for A in (1, MAX_IN - S):
            for Lp in (1, MAX_LAYERS):
                pol = (S,) + (MAX_WIDTH,) * (Lp - 1) + (A,)
                dyn = (S + A,) + (MAX_WIDTH,) * (MAX_LAYERS - 1) + (S,)
                assert admissible(MAX_K, pol, dyn, MAX_H) is None
                lds = host_plan(MAX_K, pol, dyn).lds
                if best is None or lds > best[0]:
                    best = (lds, MAX_K, pol, dyn)
    return best


# ---------------------------------------------------------------- inputs and the oracle
def make_inputs(case: Case, seed=None):
    """float64 inputs of a case: phi (D_pol,), W (K, D_dyn), s0 (K, S), eps (H, K, S)."""
    seed = SEED.get(case.name, 3) if seed is None else seed
    rng = np.random.default_rng([seed, 77])
    phi = rc.draw_phi(rng, case)
    W = np.stack([pc.draw_flat(rng, case.dyn_dims, 0.7) for _ in range(case.K)])
    s0 = rng.uniform(-0.05, 0.05, size=(case.K, case.S))
    eps = rng.normal(size=(case.H, case.K, case.S))
    return dict(phi=phi, W=W, s0=s0, eps=eps)


def oracle(case, phi, W, s0, eps, freq, dtype=torch.float64):
    """pilco_rbf_checks.rollout, unchanged, at the case's horizon.  Where no step t >= 1 is counted the cost does not
    depend on phi and its backward() raises: the gradient is then exactly zero, and is returned as such."""
    if pc.counted_steps(case.H, freq, GAMMA):
        return rc.rollout(case, phi, W, s0, eps, freq=freq, dtype=dtype)
    res = rc.rollout(case, phi, W, s0, eps, freq=freq, dtype=dtype, want_grad=False)
    res["grad"] = np.zeros(len(phi), dtype=res["states"].dtype)
    return res


_INP, _REF = {}, {}


def inputs(name):
    if name not in _INP:
        _INP[name] = make_inputs(CASE[name])
        for v in _INP[name].values():
            v.setflags(write=False)
    return _INP[name]


def reference(name, freq=None):
    """(inputs, float64 result) of a case at one of its freqs (None: the first), computed once and shared.  Read-only."""
    freq = CASE[name].freqs[0] if freq is None else freq
    if (name, freq) not in _REF:
        res = oracle(CASE[name], **inputs(name), freq=freq)
        for v in (res["grad"], res["states"], res["actions"]):
            v.setflags(write=False)
        _REF[name, freq] = res
    return inputs(name), _REF[name, freq]


def rbf_outputs(case, inp, ref):
    """Every output of the case's RBF layers over the rollout's states (the median must sit well inside (0, 1))."""
    x = torch.tensor(ref["states"][:-1].reshape(-1, case.S))
    phi = torch.tensor(np.asarray(inp["phi"]))
    outs = []
    for sl, i, o, kind, act, gamma in zip(rc.layer_slices(case), case.pol_dims[:-1], case.pol_dims[1:], case.pol_kinds,
                                          case.pol_acts, case.pol_gammas):
        th = phi[sl]
        if kind == "rbf":
            x = rc.rbf_forward(x, th.reshape(i, o), gamma)
            outs.append(x.numpy().ravel())
        else:
            x = pc._act(x @ th[:i * o].reshape(i, o) + th[i * o:], act)
    return np.concatenate(outs)


def worst_ratios(case, got, ref):
    """{quantity: error / tolerance} under the GPU bound: gradient per layer slice, states and actions against TOL * max
    |ref|, the cost against TOL * |ref|.  A zero reference (freq > H) admits only a zero."""
    out = {}
    for l, sl in enumerate(rc.layer_slices(case)):
        err, scale = np.abs(got["grad"][sl] - ref["grad"][sl]).max(), np.abs(ref["grad"][sl]).max()
        out[f"grad[{l}]"] = err / (TOL * scale) if scale else (0.0 if err == 0 else np.inf)
    for key in ("states", "actions"):
        out[key] = np.abs(got[key] - ref[key]).max() / (TOL * np.abs(ref[key]).max())
    out["cost"] = abs(got["cost"] - ref["cost"]) / (TOL * abs(ref["cost"]))
    return out


# ---------------------------------------------------------------- wrong oracles
def _fwd_only(right, wrong):
    """`wrong` going forward, the gradient of `right`."""
    return right + (wrong - right).detach()


def _bwd_only(right, wrong):
    """`right` going forward, the gradient of `wrong`."""
    return wrong + (right - wrong).detach()


def _cut(z, variant):
    """The one-trip n0 loop: output columns >= 256 (>= 128) of a layer are never written -- zero here."""
    for tag, lim in (("256", 256), ("128", 128)):
        if variant in (f"cols{tag}_fwd", f"cols{tag}_bwd") and z.shape[-1] > lim:
            mask = torch.zeros(z.shape[-1], dtype=z.dtype)
            mask[:lim] = 1.0
            return _fwd_only(z, z * mask) if variant.endswith("fwd") else _bwd_only(z, z * mask)
    return z


def _out_act(z, name, variant):
    if name == "softmax" and variant == "softmax_no_dot":
        a = torch.softmax(z, dim=-1)
        return _bwd_only(a, z * a.detach())                 # dz = a da: the Jacobian without its - a (a . da)
    return pc._act(z, name)


def variant_rollout(case, phi, W, s0, eps, freq, variant=None, gamma=GAMMA):
    """The float64 rollout with one thing wrong (variant None: nothing; then it is pilco_rbf_checks.rollout bit for bit,
    which test_pilco_dispatch_table.py asserts)."""
    H, K, dt = case.H, case.K, torch.float64
    phi_t = torch.tensor(np.asarray(phi), dtype=dt, requires_grad=True)
    W_t, s, eps_t = (torch.tensor(np.asarray(v), dtype=dt) for v in (W, s0, eps))
    if variant == "next_draw":
        W_t = torch.roll(W_t, -1, dims=0)                   # particle i runs draw (i + 1) % K
    states, actions = [s], []
    cost = -pc.reward(case.reward, s, 0).mean()
    discount, dropped = 1.0, 0.0
    n_pol = len(case.pol_acts)
    for t in range(1, H + 1):
        x = s
        for l, (sl, i, o, kind, act, g) in enumerate(zip(rc.layer_slices(case), case.pol_dims[:-1], case.pol_dims[1:],
                                                         case.pol_kinds, case.pol_acts, case.pol_gammas)):
            th = phi_t[sl]
            if kind == "rbf":
                d2 = ((x.unsqueeze(-1) - th.reshape(i, o)) ** 2).sum(dim=1)
                x = torch.exp(-1 * g * _cut(d2, variant)) if variant and variant.startswith("cols") else \
                    rc.rbf_forward(x, th.reshape(i, o), g)
            else:
                z = _cut(x @ th[:i * o].reshape(i, o) + th[i * o:], variant)
                x = _out_act(z, act, variant) if l == n_pol - 1 else pc._act(z, act)
        a = x
        y, off = torch.cat([s, a], dim=1), 0
        for i, o, act in zip(case.dyn_dims[:-1], case.dyn_dims[1:], case.dyn_acts):
            w = W_t[:, off:off + i * o].reshape(-1, i, o)
            b = W_t[:, off + i * o:off + (i + 1) * o]
            off += (i + 1) * o
            y = pc._act(_cut(torch.einsum("ki,kio->ko", y, w) + b, variant), act)
        ym = y[:THREADS // case.S] if variant == "staging_cut" else y     # particles past the first trip left out
        m = ym.mean(dim=0)
        sd = torch.sqrt(((ym - m) ** 2).mean(dim=0))
        if variant == "sd_k_minus_1":
            sd = sd * np.sqrt(K / (K - 1.0))
        if variant == "sd_detached":
            sd = sd.detach()
        s = m + sd * eps_t[t % H if variant == "eps_next" else t - 1]
        states.append(s)
        actions.append(a)
        counted = t % freq == 0 or (variant == "last_counted" and t == H)
        if counted:
            discount = gamma ** t if variant == "gamma_t" else discount * gamma
            term = discount * pc.reward(case.reward, s, t).mean()
            cost = cost - term
            if variant == "cost_255" and t > 255:           # the cost loop alone stops early: the gradient is right
                dropped += float(term.detach())
    grad = np.zeros(len(phi))
    if cost.requires_grad:
        cost.backward()
        grad = phi_t.grad.numpy().copy()
    return dict(cost=float(cost.detach()) + dropped, grad=grad, states=torch.stack(states).detach().numpy(),
                actions=torch.stack(actions).detach().numpy())


def _widest(c):
    return max(c.pol_dims[1:] + c.dyn_dims[1:])


# variant -> does it apply to (case, freq): where it does it must miss the GPU bound
VARIANTS = {
    "sd_k_minus_1": lambda c, f: True,
    "sd_detached": lambda c, f: bool(pc.counted_steps(c.H, f, GAMMA)),       # the states are right; only a gradient shows it
    "eps_next": lambda c, f: True,
    "gamma_t": lambda c, f: f > 1 and bool(pc.counted_steps(c.H, f, GAMMA)),
    "last_counted": lambda c, f: c.H % f != 0,
    "next_draw": lambda c, f: True,
    "staging_cut": lambda c, f: c.K > THREADS // c.S,
    "cols256_fwd": lambda c, f: _widest(c) > 256,
    "cols256_bwd": lambda c, f: _widest(c) > 256 and bool(pc.counted_steps(c.H, f, GAMMA)),
    "cols128_fwd": lambda c, f: _widest(c) > 128,
    "cols128_bwd": lambda c, f: _widest(c) > 128 and bool(pc.counted_steps(c.H, f, GAMMA)),
    "cost_255": lambda c, f: any(t > 255 for t, _ in pc.counted_steps(c.H, f, GAMMA)),
    "softmax_no_dot": lambda c, f: c.pol_out == "softmax" and bool(pc.counted_steps(c.H, f, GAMMA)),
}


def applies(variant):
    """[(case name, freq)] a wrong oracle applies to."""
    return [(c.name, f) for c in NEW_CASES for f in c.freqs if VARIANTS[variant](c, f)]


if __name__ == "__main__":      # the figures of profiles/pilco_matrix/float32_standin.txt
    print("float32 restatement against the float64 one: worst error / (1e-5 max |ref|), min_sd")
    for c in NEW_CASES:
        for f in c.freqs:
            inp, ref = reference(c.name, f)
            r32 = oracle(c, **inp, freq=f, dtype=torch.float32)
            r = {k: v * TOL / 1e-5 for k, v in worst_ratios(c, r32, ref).items()}
            print(f"{c.name} freq {f}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f", min_sd {ref['min_sd']:.4f}, "
                  f"max |s| {np.abs(ref['states']).max():.3f}")
    print("wrong oracles against the right one: worst error / tolerance (must be > 1)")
    for variant in VARIANTS:
        for name, f in applies(variant):
            inp, ref = reference(name, f)
            r = worst_ratios(CASE[name], variant_rollout(CASE[name], **inp, freq=f, variant=variant), ref)
            k = max(r, key=r.get)
            print(f"{variant} on {name} freq {f}: {r[k]:.3g} ({k})")
