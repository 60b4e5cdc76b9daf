"""SGLD with P chains per launch (pyz_sgld_chains_step / _run, SGLD's n_chains): the cases, their data, the float64
restatement of one P-chain step and the comparison the GPU test uses (a plain module).

One P-chain step is P single-chain SGLD steps on one shared batch: chain c from row c of the (P, D) state, with the Philox
seed `seed + c`.  `ref_chains_step` says exactly that on top of step_cases.ref_step, and `compare_chains_step` is
step_cases.compare_step chain by chain -- the tolerances are the ones of the single-chain step, nothing is added here.
`MUTATIONS` are the wrong kernels the comparison has to reject (tests/test_sgld_chains_host.py runs them on the CPU)."""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import step_cases as sc
from dense_cases import batch_rows, case_data
from oracle import philox as o_philox
from step_cases import StepCase

R, T, G, LN, SM = "relu", "tanh", "sigmoid", "linear", "softmax"
N_STEPS = sc.N_STEPS
VARIANTS = sc.VARIANTS["sgld"]            # zeros, philox (the stream injected), device (the kernel draws it)


class ChainsCase(NamedTuple):
    step: StepCase                         # shape, batch, lr, n0 = 3, seed, alignment of the state buffers
    P: int

    @property
    def name(self) -> str:
        return f"{self.step.name}_p{self.P}"

    @property
    def D(self) -> int:
        return sum((k + 1) * n for k, n in zip(self.step.dims[:-1], self.step.dims[1:]))


def _c(name, dims, acts, loss, batch, P, **kw):
    return ChainsCase(StepCase(name, tuple(dims), tuple(acts), loss, batch, **kw), P)


# D = sum (K + 1) N.  Fused = a last layer of at most 32 units (per-particle losses from the weight-gradient launch), else
# the per-layer weight gradients and k_loss_finalize.  One workgroup of the update covers 256 groups = 1024 elements.
CASES = [
    _c("f_d404", (20, 16, 4), (R, SM), "scce", 14, 5, aligned=True),                 # D % 4 = 0, every row aligned
    _c("f_d25_odd", (2, 3, 4), (R, SM), "scce", 5, 2),                               # D % 4 = 1, odd batch, 4 bytes off
    _c("f_d66_gathered", (5, 7, 3), (T, SM), "scce", 11, 5, gathered=True, aligned=True),   # D % 4 = 2, ragged N, rows 0, 2, 4 aligned
    _c("f_d83_mse", (6, 8, 3), (T, LN), "mse", 8, 1),                                # D % 4 = 3, MSE, one chain
    _c("f_d67_bce", (9, 6, 1), (T, G), "bce", 13, 5),                                # BCE head
    _c("u_d99", (2, 33), (SM,), "scce", 9, 2, aligned=True),                         # a last layer of 33: the finalise kernel
    _c("u_d165_mse", (4, 33), (LN,), "mse", 16, 5),                                  # D % 4 = 1, unfused, MSE
    _c("u_d218_gathered", (3, 5, 33), (T, SM), "scce", 31, 1, gathered=True),        # D % 4 = 2, unfused, gathered
    _c("u_d1100", (12, 20, 40), (T, SM), "scce", 37, 5, data_seed=2),                # 275 groups: two workgroups per chain
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def coverage():
    """What the case list has to reach (tests/test_sgld_chains_host.py asserts every entry)."""
    return {
        "P": {c.P for c in CASES},
        "D % 4": {c.D % 4 for c in CASES},
        "more than one workgroup per chain": any(c.D > sc.BLOCK and c.P > 1 for c in CASES),
        "aligned": {c.step.aligned for c in CASES},
        "odd batch": any(c.step.batch % 2 for c in CASES),
        "gathered with a ragged N": any(c.step.gathered and any(n % 32 for n in c.step.dims[1:]) for c in CASES),
        "fused": {c.step.fused for c in CASES},
        "last layer of 33": any(c.step.dims[-1] == 33 for c in CASES),
        "loss": {c.step.loss for c in CASES},
        "unaligned rows behind an aligned first row": any(c.step.aligned and c.D % 4 and c.P > 1 for c in CASES),
    }


# ---------------------------------------------------------------- data
class ChainsData(NamedTuple):
    step: sc.StepData          # x, y, idx, rows, ys of the shared batch (theta0 / mean0 / sq0: chain 0's)
    theta0: np.ndarray         # (P, D) float32, a different start per chain
    mean0: np.ndarray          # (P, D) near theta0
    sq0: np.ndarray            # (P, D) >= mean0^2


def chains_data(case: ChainsCase) -> ChainsData:
    """dense_cases.case_data with P particles (the batch is the one the single-chain case has) and, per chain, the
    non-zero starting moments step_cases.step_data gives its one chain."""
    st, P = case.step, case.P
    dense = st.dense._replace(P=P)
    x, y, idx, thetas = case_data(dense)
    rows, ys = batch_rows(dense, x, y, idx)
    D = thetas.shape[1]
    rng = np.random.default_rng(sum(map(ord, case.name)) + 7919 * (st.data_seed + 1))
    rms = np.sqrt(np.mean(thetas.astype(np.float64) ** 2, axis=1, keepdims=True))
    mean0 = (thetas + 0.1 * rms * rng.normal(size=(P, D))).astype(np.float32)
    sq0 = (mean0.astype(np.float64) ** 2 + (0.05 * rms * (1.0 + rng.uniform(size=(P, D)))) ** 2).astype(np.float32)
    step = sc.StepData(x, y, idx, rows, ys, thetas[0], mean0[0], sq0[0], np.zeros((2, D), np.float32), np.zeros(D, np.float32),
                       None, None)
    return ChainsData(step, thetas, mean0, sq0)


def initial_state(data: ChainsData) -> dict:
    return {"theta": data.theta0.copy(), "mean": data.mean0.copy(), "sq": data.sq0.copy()}


def chain_case(case: ChainsCase, c: int) -> StepCase:
    """The single-chain case chain c is: the same step with the seed seed + c."""
    return case.step._replace(seed=case.step.seed + c)


def chain_state(s: dict, c: int) -> dict:
    return {k: np.asarray(v)[c] for k, v in s.items()}


def injected_noise(case: ChainsCase, variant: str, k: int) -> Optional[np.ndarray]:
    """The (P, D) float32 matrix a step is given as unit_noise (None: the device draws it): row c = chain c's stream."""
    if variant == "device":
        return None
    return np.stack([sc.injected_noise(chain_case(case, c), "sgld", variant, k) for c in range(case.P)])


# ---------------------------------------------------------------- one P-chain step, restated (any dtype, wrong variants)
MUTATIONS = (
    "every chain on seed `seed`",
    "row stride D rounded up to 4",
    "count n + 1",
    "moments from the old theta",
    "chain c's loss from chain 0",
)


def mutation_applies(case: ChainsCase, variant: str, mutation: str) -> bool:
    if mutation == "every chain on seed `seed`":
        return case.P > 1 and variant != "zeros"
    if mutation == "row stride D rounded up to 4":
        return case.P > 1 and case.D % 4 != 0
    if mutation == "chain c's loss from chain 0":
        return case.P > 1
    return True


def ref_chains_step(case: ChainsCase, data: ChainsData, variant: str, k: int, s0: dict, dtype=np.float64, mutation=None) -> dict:
    """Step k (count n0 + k) of all P chains from the (P, D) state s0: step_cases.ref_step(chain c's case, the shared
    batch, "sgld", variant, k, row c of s0).  Returns theta / mean / sq (P, D) and loss (P,)."""
    P, D = case.P, case.D
    if mutation == "row stride D rounded up to 4":
        # the gradient pass is the right one (gradients of the real rows, at stride D in the gradient buffer); the update
        # takes row c of the state AND of the gradients at c * D4 of the flat buffers and writes there; what lies past
        # the end of the (P, D) buffers does not exist for the caller
        D4 = 4 * ((D + 3) // 4)
        flat = {key: np.concatenate([np.asarray(s0[key], dtype=dtype).reshape(-1), np.zeros(P * D4 - P * D, dtype=dtype)])
                for key in ("theta", "mean", "sq")}
        grad_flat = np.zeros(P * D4, dtype=dtype)
        losses = []
        for c in range(P):
            loss, g = sc._gradient(np.asarray(s0["theta"], dtype=dtype)[c], data.step, case.step.spec, dtype, None)
            grad_flat[c * D:(c + 1) * D] = g
            losses.append(loss)
        lr, n = dtype(case.step.lr), dtype(case.step.n0 + k)
        for c in range(P):
            sl = slice(c * D4, c * D4 + D)
            th = flat["theta"][sl] + (-lr) * (grad_flat[sl] + lr * _noise(case, c, variant, k, dtype))
            flat["theta"][sl] = th
            flat["mean"][sl] = (flat["mean"][sl] * n + th) / (n + dtype(1.0))
            flat["sq"][sl] = (flat["sq"][sl] * n + th ** 2) / (n + dtype(1.0))
        out = {key: flat[key][:P * D].reshape(P, D).copy() for key in flat}
        out["loss"] = np.array(losses, dtype=dtype)
        return out
    outs = []
    for c in range(P):
        cc = case.step if mutation == "every chain on seed `seed`" else chain_case(case, c)
        o = sc.ref_step(cc, data.step, "sgld", variant, k, chain_state(s0, c), dtype,
                        "moments with count n + 1" if mutation == "count n + 1" else None)
        if mutation == "moments from the old theta":
            n, th0 = dtype(case.step.n0 + k), np.asarray(s0["theta"], dtype=dtype)[c]
            o["mean"] = (np.asarray(s0["mean"], dtype=dtype)[c] * n + th0) / (n + dtype(1.0))
            o["sq"] = (np.asarray(s0["sq"], dtype=dtype)[c] * n + th0 ** 2) / (n + dtype(1.0))
        outs.append(o)
    out = {key: np.stack([np.asarray(o[key]) for o in outs]) for key in ("theta", "mean", "sq")}
    out["loss"] = np.array([outs[0 if mutation == "chain c's loss from chain 0" else c]["loss"] for c in range(P)], dtype=dtype)
    return out


def _noise(case: ChainsCase, c: int, variant: str, k: int, dtype):
    if variant == "zeros":
        return np.zeros(case.D, dtype=dtype)
    z = o_philox.normal(case.step.seed + c, sc.STREAM["sgld"], case.step.n0 + k, case.D)
    return (z.astype(np.float32) if variant == "philox" else z).astype(dtype)


def as_stored(out: dict) -> dict:
    return {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}


# ---------------------------------------------------------------- the comparison
def compare_chains_step(case: ChainsCase, k: int, s0: dict, got: dict, ref: dict, what: str = "") -> dict:
    """step_cases.compare_step for every chain: row c of `got` against row c of the float64 reference `ref`, both from
    row c of s0.  Raises AssertionError on the first bound a chain misses; returns quantity -> the largest error over
    tolerance of any chain."""
    rep = {}
    for c in range(case.P):
        r = sc.compare_step(chain_case(case, c), "sgld", k, chain_state(s0, c), chain_state(got, c), chain_state(ref, c),
                            what=f"{what}chain {c} of {case.P}: ")
        for q, v in r.items():
            rep[q] = max(rep.get(q, 0.0), v)
    return rep


# ---------------------------------------------------------------- the run
RUN_SIZES = (8, 8, 5, 8, 8, 5, 8)        # 21 rows per epoch: ragged, two epoch changes in seven steps


def run_lrs(n_steps: int, first: int = 0):
    """A learning rate per step, all different (a run that took the wrong table entry would show)."""
    return [float(np.float32(0.05 / (1.0 + 0.25 * (first + s)))) for s in range(n_steps)]
