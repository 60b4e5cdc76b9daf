"""BBB lanes (pyz_bbb_lanes_step / _run, BBB's lanes): the cases, the float64 restatement of one P-lane step and the
comparison the GPU test uses (a plain module).

A P-lane step is P single BBB steps on one shared batch: lane c from row c of the (P, D) state with its own lr, alpha and
scalar prior, and the Philox seed `seed + c * stride`, stride 0 or 1.  The cases are the nine shapes of sgld_chains_checks
(every D % 4, fused and 33-unit unfused heads, scce / mse / bce, gathered rows, aligned and 4-bytes-off buffers, D = 1100
for two blocks per lane) with

    lane c = case.step._replace(bbb_lr = bbb_lr (1 + c / 4), alpha = alpha_c, prior = (pm + c / 8, pr - c / 4),
                                seed = seed + c * stride)

alpha_c = alpha (1 + c / 2): all different and none zero -- except in ZERO_ALPHA, where lane 2 has alpha = 0 (the update
then is plain SGD on the sampled weights and the cost is the data loss).  The cases in PRIOR_VEC give the shared
per-element prior vectors (the lanes' scalars are passed too and must be ignored).  `ref_bbb_lanes_step` says the above on
top of step_cases.ref_step, and `compare_bbb_lanes_step` is step_cases.compare_step lane by lane -- no tolerance is added or
changed here.  `MUTATIONS` are the wrong kernels the comparison has to reject (tests/test_bbb_lanes_host.py runs them on
the CPU)."""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import step_cases as sc
import sgld_chains_checks as cc
from sgld_chains_checks import ChainsCase, chain_state

STRIDES = (0, 1)
N_STEPS = sc.N_STEPS
VARIANTS = sc.VARIANTS["bbb"]              # philox (the stream injected), device (the kernel draws it)
PRIOR_VEC = ("f_d66_gathered_p5", "u_d99_p2")
ZERO_ALPHA = ("f_d67_bce_p5", 2)           # (case, lane)

CASES = [ChainsCase(c.step._replace(prior_vec=c.name in PRIOR_VEC), c.P) for c in cc.CASES]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASES) == 9 and {c.P for c in CASES} == {1, 2, 5} and all(n in CASE_BY_NAME for n in PRIOR_VEC + ZERO_ALPHA[:1])


class LaneTables(NamedTuple):
    lr: np.ndarray             # float32 (P,) each
    alpha: np.ndarray
    prior_mean: np.ndarray
    prior_rho: np.ndarray


def lane_tables(case: ChainsCase) -> LaneTables:
    """The four host tables of the case's lanes; every entry is exact in float32 (the cases' numbers are dyadic)."""
    st, P = case.step, case.P
    lr = [st.bbb_lr * (1.0 + c / 4.0) for c in range(P)]
    alpha = [st.alpha * (1.0 + c / 2.0) for c in range(P)]
    if case.name == ZERO_ALPHA[0]:
        alpha[ZERO_ALPHA[1]] = 0.0
    pm = [st.prior[0] + c / 8.0 for c in range(P)]
    pr = [st.prior[1] - c / 4.0 for c in range(P)]
    t = LaneTables(*(np.array(v, dtype=np.float32) for v in (lr, alpha, pm, pr)))
    for got, want in zip(t, (lr, alpha, pm, pr)):
        assert np.array_equal(got.astype(np.float64), want)
    return t


def lane_case(case: ChainsCase, c: int, stride: int, tables: Optional[LaneTables] = None) -> sc.StepCase:
    """The single BBB step lane c is."""
    t = lane_tables(case) if tables is None else tables
    return case.step._replace(bbb_lr=float(t.lr[c]), alpha=float(t.alpha[c]), prior=(float(t.prior_mean[c]), float(t.prior_rho[c])),
                              seed=case.step.seed + c * stride)


# ---------------------------------------------------------------- data
class LanesData(NamedTuple):
    step: sc.StepData          # the shared batch; pm_vec / pr_vec: the shared prior vectors of a PRIOR_VEC case
    mu0: np.ndarray            # (P, D) float32, a different start per lane
    rho0: np.ndarray           # (P, D) uniform in [-3, 1] (step_cases.step_data's range)


_DATA = {}


def lanes_data(case: ChainsCase) -> LanesData:
    """sgld_chains_checks.chains_data (the batch and a start per lane) with rho0 per lane and, where the case asks, the
    prior vectors step_cases.step_data draws.  Computed once per case, shared, never written to."""
    if case.name not in _DATA:
        data = cc.chains_data(case)
        P, D = data.theta0.shape
        rng = np.random.default_rng(sum(map(ord, case.name)) + 104729)
        rho0 = rng.uniform(-3.0, 1.0, size=(P, D)).astype(np.float32)
        pm_vec = pr_vec = None
        if case.step.prior_vec:
            pm_vec = rng.uniform(-0.5, 0.5, size=D).astype(np.float32)
            pr_vec = rng.uniform(0.25, 1.5, size=D).astype(np.float32)
        mu0 = data.theta0.copy()
        for a in (mu0, rho0, pm_vec, pr_vec):
            if a is not None:
                a.setflags(write=False)
        _DATA[case.name] = LanesData(data.step._replace(pm_vec=pm_vec, pr_vec=pr_vec), mu0, rho0)
    return _DATA[case.name]


def initial_state(data: LanesData) -> dict:
    return {"mu": data.mu0.copy(), "rho": data.rho0.copy(), "w": np.zeros_like(data.mu0)}


def injected_noise(case: ChainsCase, variant: str, k: int, stride: int) -> Optional[np.ndarray]:
    """The (P, D) float32 matrix a step is given as eps (None: the device draws it): row c = lane c's stream."""
    if variant == "device":
        return None
    return np.stack([sc.injected_noise(lane_case(case, c, stride), "bbb", variant, k) for c in range(case.P)])


# ---------------------------------------------------------------- one P-lane step, restated (any dtype, wrong variants)
MUTATIONS = (
    "every lane on lane 0's lr",
    "every lane on lane 0's alpha",
    "lane c with lane P-1-c's prior",
    "stride swapped",
    "a lane's KL taken from lane 0",
)


def mutation_applies(case: ChainsCase, variant: str, stride: int, mutation: str) -> bool:
    if case.P < 2:
        return False
    if mutation == "lane c with lane P-1-c's prior":
        return not case.step.prior_vec          # the vectors are shared: the scalars are not read
    return True


def ref_bbb_lanes_step(case: ChainsCase, data: LanesData, variant: str, k: int, s0: dict, stride: int, dtype=np.float64,
                       mutation=None) -> dict:
    """Step k (Philox step n0 + k) of all P lanes from the (P, D) state s0: row by row step_cases.ref_step(lane c's case, the
    shared batch, "bbb", variant, k, row c of s0).  Returns mu / rho / w (P, D), cost (P, 3) and kl_abs (P,)."""
    P = case.P
    t = lane_tables(case)
    if mutation == "every lane on lane 0's lr":
        t = t._replace(lr=np.full(P, t.lr[0], dtype=np.float32))
    elif mutation == "every lane on lane 0's alpha":
        t = t._replace(alpha=np.full(P, t.alpha[0], dtype=np.float32))
    elif mutation == "lane c with lane P-1-c's prior":
        t = t._replace(prior_mean=t.prior_mean[::-1].copy(), prior_rho=t.prior_rho[::-1].copy())
    elif mutation == "stride swapped":
        stride = 1 - stride
    outs = [sc.ref_step(lane_case(case, c, stride, t), data.step, "bbb", variant, k, chain_state(s0, c), dtype) for c in range(P)]
    out = {key: np.stack([np.asarray(o[key]) for o in outs]) for key in ("mu", "rho", "w", "cost")}
    out["kl_abs"] = np.array([o["kl_abs"] for o in outs], dtype=np.float64)
    if mutation == "a lane's KL taken from lane 0":
        for c in range(1, P):
            kl = out["cost"][0][2]
            out["cost"][c] = np.array([out["cost"][c][1] + dtype(t.alpha[c]) * kl, out["cost"][c][1], kl], dtype=dtype)
    return out


def as_stored(out: dict) -> dict:
    return {k: (v if k == "kl_abs" else np.asarray(v, dtype=np.float32)) for k, v in out.items()}


def compare_bbb_lanes_step(case: ChainsCase, k: int, s0: dict, got: dict, ref: dict, stride: int, what: str = "") -> dict:
    """step_cases.compare_step for every lane: row c of `got` against row c of the float64 reference `ref`, both from row c
    of s0.  Raises AssertionError on the first bound a lane misses; returns quantity -> the largest error over tolerance."""
    rep = {}
    for c in range(case.P):
        r = sc.compare_step(lane_case(case, c, stride), "bbb", k, chain_state(s0, c), chain_state(got, c), chain_state(ref, c),
                            what=f"{what}lane {c} of {case.P}: ")
        for q, v in r.items():
            rep[q] = max(rep.get(q, 0.0), v)
    return rep


# ---------------------------------------------------------------- which steps the GPU test takes
# Every case takes the three steps n0, n0 + 1, n0 + 2 EACH FROM ITS START (three Philox steps, three draws of eps).  Walking
# them one after the other is kept for the cases in WALK only: at the lane rates above (0.5 .. 1.0, set for these shapes by
# SGLD's cases, not by BBB's) the float64 reference itself diverges on four of the nine shapes -- its data loss grows
# tenfold per step and rho runs to -10 and far below within two steps --, and from such a state float32 cannot form
# (w - mu) / sigma to the accuracy compare_step's bound on log q - log p presumes: a float32 NumPy restatement of the step
# misses that bound there as well (3 times the tolerance at step 2 of f_d404_p5).  That is the number format, not a kernel.
# WALK is decided by the reference alone: every lane's rho stays at or above WALK_RHO_MIN (sigma >= 0.0067) through the three steps
# (tests/test_bbb_lanes_host.py asserts it, and that the float32 restatement passes the walk on exactly these).
WALK_RHO_MIN = -5.0
WALK = ("f_d66_gathered_p5", "f_d83_mse_p1", "f_d67_bce_p5", "u_d218_gathered_p1", "u_d1100_p5")
assert all(n in CASE_BY_NAME for n in WALK)


# ---------------------------------------------------------------- the run
RUN_SIZES = (9, 9, 5, 9, 9, 5, 9)          # 23 rows per epoch: ragged, two epoch changes in seven steps
