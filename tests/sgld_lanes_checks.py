"""SGLD lanes (pyz_sgld_lanes_step / _run, SGLD's lanes): the cases, the float64 restatement of one P-lane step and the
comparison the GPU test uses (a plain module).

A P-lane step is P single-chain SGLD steps on one shared batch: lane c from row c of the (P, D) state with the rate lr_c
and the Philox seed `seed + c * stride`, stride 0 or 1.  The cases are the ones of sgld_chains_checks (same shapes, data and
starts) with the lane rates lr_c = lr (1 + c / 4): all different, none below the case's lr, so step_cases.compare_step's
increment test keeps the sensitivity it has there.  `ref_lanes_step` says the above on top of step_cases.ref_step, and
`compare_lanes_step` is step_cases.compare_step lane by lane -- no tolerance is added here.  `MUTATIONS` are the wrong
kernels the comparison has to reject (tests/test_sgld_lanes_host.py runs them on the CPU)."""

from __future__ import annotations

from typing import Optional

import numpy as np

import step_cases as sc
from sgld_chains_checks import CASE_BY_NAME, CASES, N_STEPS, VARIANTS, ChainsCase, ChainsData, as_stored, chain_state, chains_data, initial_state  # noqa: F401

STRIDES = (0, 1)


def lane_rates(case: ChainsCase) -> np.ndarray:
    """float32 (P,): lr_c = lr (1 + c / 4) (exact in float32 for the cases' lr = 0.5)."""
    r = np.array([case.step.lr * (1.0 + c / 4.0) for c in range(case.P)], dtype=np.float32)
    assert np.array_equal(r.astype(np.float64), [case.step.lr * (1.0 + c / 4.0) for c in range(case.P)])
    return r


def lane_case(case: ChainsCase, c: int, stride: int, rates=None) -> sc.StepCase:
    """The single-chain case lane c is: the same step with the rate lr_c and the seed seed + c * stride."""
    rates = lane_rates(case) if rates is None else rates
    return case.step._replace(lr=float(rates[c]), seed=case.step.seed + c * stride)


def injected_noise(case: ChainsCase, variant: str, k: int, stride: int) -> Optional[np.ndarray]:
    """The (P, D) float32 matrix a step is given as unit_noise (None: the device draws it): row c = lane c's stream."""
    if variant == "device":
        return None
    return np.stack([sc.injected_noise(lane_case(case, c, stride), "sgld", variant, k) for c in range(case.P)])


MUTATIONS = (
    "every lane on lane 0's rate",
    "lane c on lane P-1-c's rate",
    "stride 1 where 0 was asked",
    "stride 0 where 1 was asked",
)


def mutation_applies(case: ChainsCase, variant: str, stride: int, mutation: str) -> bool:
    if case.P < 2:
        return False
    if mutation == "stride 1 where 0 was asked":
        return stride == 0 and variant != "zeros"
    if mutation == "stride 0 where 1 was asked":
        return stride == 1 and variant != "zeros"
    return True


def ref_lanes_step(case: ChainsCase, data: ChainsData, variant: str, k: int, s0: dict, stride: int, dtype=np.float64,
                   mutation=None, rates=None) -> dict:
    """Step k (count n0 + k) of all P lanes from the (P, D) state s0: row by row step_cases.ref_step(the step with lr = lr_c
    and seed = seed + c * stride, the shared batch, "sgld", variant, k, row c of s0).  Returns theta / mean / sq (P, D) and
    loss (P,)."""
    P = case.P
    rates = lane_rates(case) if rates is None else np.asarray(rates, dtype=np.float32)
    if mutation == "every lane on lane 0's rate":
        rates = np.full(P, rates[0], dtype=np.float32)
    elif mutation == "lane c on lane P-1-c's rate":
        rates = rates[::-1].copy()
    elif mutation in ("stride 1 where 0 was asked", "stride 0 where 1 was asked"):
        stride = 1 - stride
    outs = [sc.ref_step(case.step._replace(lr=float(rates[c]), seed=case.step.seed + c * stride), data.step, "sgld", variant, k,
                        chain_state(s0, c), dtype) for c in range(P)]
    out = {key: np.stack([np.asarray(o[key]) for o in outs]) for key in ("theta", "mean", "sq")}
    out["loss"] = np.array([o["loss"] for o in outs], dtype=dtype)
    return out


def compare_lanes_step(case: ChainsCase, k: int, s0: dict, got: dict, ref: dict, stride: int, what: str = "", rates=None) -> dict:
    """step_cases.compare_step for every lane: row c of `got` against row c of the float64 reference `ref`, both from row c
    of s0.  Raises AssertionError on the first bound a lane misses; returns quantity -> the largest error over tolerance."""
    rep = {}
    for c in range(case.P):
        r = sc.compare_step(lane_case(case, c, stride, rates), "sgld", k, chain_state(s0, c), chain_state(got, c),
                            chain_state(ref, c), what=f"{what}lane {c} of {case.P}: ")
        for q, v in r.items():
            rep[q] = max(rep.get(q, 0.0), v)
    return rep


# ---------------------------------------------------------------- the run
def run_rate_table(n_steps: int, P: int) -> np.ndarray:
    """float32 (n_steps, P), every entry different (a run that took another step's row or another lane's column would show)."""
    t = np.array([[0.05 / (1.0 + 0.25 * s + 0.0625 * c) for c in range(P)] for s in range(n_steps)], dtype=np.float32)
    assert len(set(t.reshape(-1).tolist())) == t.size
    return t
