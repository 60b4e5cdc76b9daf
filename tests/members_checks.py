"""SGD / SWAG with P members per launch (pyz_sgd_members_step / _run, pyz_swag_members_step / _run; the optimizers'
n_members): the cases, their data, the float64 restatement of one P-member step and the comparison the GPU test uses (a
plain module).

One P-member step is P single-model steps on one shared batch: member c from row c of the (P, D) state (SWAG: and block c
of the (P, k, D) deviations, k = 2).  `ref_members_step` says exactly that on top of step_cases.ref_step, and
`compare_members_step` is step_cases.compare_step member by member -- the tolerances are the ones of the single-model
step, nothing is added; for SGD rows, whose "mean" step_cases does not know, the row must hold the bits of the stored new
weights after a hit step and its old bits after a miss.  `MUTATIONS` are the wrong kernels the comparison has to reject
(tests/test_members_host.py runs them on the CPU)."""

from __future__ import annotations

import numpy as np

import sgld_chains_checks as cc
import step_cases as sc

MODES = ("sgd", "swag")
N_STEPS = sc.N_STEPS
K_DEV = 2                                   # deviation rows per member in the step cases
SWAG_STEPS = sc.SWAG_STEPS                  # update into row 1; no update; update with no row
SGD_HITS = (True, False, True)              # hit, miss, hit

MembersCase = cc.ChainsCase                 # (step: StepCase, P); name, D
CASES = [MembersCase(c.step, c.P) for c in cc.CASES]      # the shapes of the SGLD-chains list
CASE_BY_NAME = {c.name: c for c in CASES}


def coverage():
    """What the case list has to reach (tests/test_members_host.py asserts every entry)."""
    cov = {
        "P": {c.P for c in CASES},
        "D % 4": {c.D % 4 for c in CASES},
        "more than one workgroup per member": any(c.D > sc.BLOCK and c.P > 1 for c in CASES),
        "aligned": {c.step.aligned for c in CASES},
        "odd batch": any(c.step.batch % 2 for c in CASES),
        "gathered with a ragged N": any(c.step.gathered and any(n % 32 for n in c.step.dims[1:]) for c in CASES),
        "fused": {c.step.fused for c in CASES},
        "last layer of 33": any(c.step.dims[-1] == 33 for c in CASES),
        "loss": {c.step.loss for c in CASES},
        "unaligned rows behind an aligned first row": any(c.step.aligned and c.D % 4 and c.P > 1 for c in CASES),
        # member m's deviation row 1 (the one the step cases write) starts (m * K_DEV + 1) * D floats behind the buffer,
        # which itself starts on a 16-byte boundary or one float behind one: rows of both alignments in one launch
        "deviation rows of both alignments in one launch": any(
            len({((0 if c.step.aligned else 1) + (m * K_DEV + 1) * c.D) % 4 == 0 for m in range(c.P)}) == 2 for c in CASES),
        "modes": set(MODES),
        "SWAG steps": set(SWAG_STEPS),
        "SGD hits": set(SGD_HITS),
    }
    return cov


# ---------------------------------------------------------------- data
def members_data(case) -> cc.ChainsData:
    """sgld_chains_checks.chains_data: the shared batch and, per member, a start with non-zero moments."""
    return cc.chains_data(case)


def initial_state(case, mode: str, data: cc.ChainsData) -> dict:
    s = {"theta": data.theta0.copy(), "mean": data.mean0.copy()}
    if mode == "swag":
        rng = np.random.default_rng(sum(map(ord, case.name)) + 104729)
        s["sq"] = data.sq0.copy()
        s["dev"] = rng.normal(size=(case.P, K_DEV, case.D)).astype(np.float32)
    return s


def member_state(s: dict, c: int) -> dict:
    return {k: np.asarray(v)[c] for k, v in s.items()}


def step_flags(mode: str, k: int):
    """(hit, deviation column or None) of step k."""
    if mode == "swag":
        return SWAG_STEPS[k]
    return SGD_HITS[k], None


# ---------------------------------------------------------------- the run's rules (k_members_update with freq > 0)
def run_hit(n: int, freq: int) -> bool:
    return n % freq == 0


def run_column(n: int, freq: int, k: int) -> int:
    return min((n + freq - 1) // freq, k - 1)


# ---------------------------------------------------------------- one P-member step, restated (any dtype, wrong variants)
MUTATIONS = (
    "row stride D rounded up to 4",
    "count n + 1",
    "deviation against the old mean",
    "moments written on a non-hit step",
    "member c's deviation written into member 0's block",
    "deviation column stride k D instead of D",
    "member c's loss from member 0",
    "SGD mean copied on a miss step",
)


def mutation_applies(case, mode: str, k: int, mutation: str) -> bool:
    hit, col = step_flags(mode, k)
    if mutation == "row stride D rounded up to 4":
        # on a hit step: there the misplaced rows meet the moments of OTHER elements.  On a miss step state and gradient
        # shift together, every element but the first c (D4 - D) of member c still takes its own gradient, and whether
        # those few stand out of their block's tolerance is up to the data; every case has hit steps around its miss step
        return case.P > 1 and case.D % 4 != 0 and hit
    if mutation == "member c's loss from member 0":
        return case.P > 1
    if mutation == "count n + 1":
        return mode == "swag" and hit
    if mutation == "deviation against the old mean":
        return mode == "swag" and hit and col is not None
    if mutation == "moments written on a non-hit step":
        return mode == "swag" and not hit
    if mutation == "member c's deviation written into member 0's block":
        return mode == "swag" and hit and col is not None and case.P > 1
    if mutation == "deviation column stride k D instead of D":
        return mode == "swag" and hit and col is not None and col > 0
    if mutation == "SGD mean copied on a miss step":
        return mode == "sgd" and not hit
    raise KeyError(mutation)


def _update(mode, hit, col, th0, g, mu0, sq0, lr, n, dt):
    """The two arms of k_members_update on arrays: (theta, mean, sq, deviation or None)."""
    th = th0 - lr * g
    if not hit:
        return th, mu0, sq0, None
    if mode == "sgd":
        return th, th, sq0, None
    mu = (mu0 * n + th) / (n + dt(1.0))
    sq = (sq0 * n + th ** 2) / (n + dt(1.0))
    return th, mu, sq, (th - mu if col is not None else None)


def ref_members_step(case, data: cc.ChainsData, mode: str, k: int, s0: dict, dtype=np.float64, mutation=None) -> dict:
    """Step k (count n0 + k) of all P members from the state s0: step_cases.ref_step(the member's case, the shared batch,
    mode, "plain", k, row c of s0).  Returns theta / mean (P, D), SWAG: sq (P, D) and dev (P, K_DEV, D), and loss (P,)."""
    P, D, dt = case.P, case.D, dtype
    hit, col = step_flags(mode, k)
    swag = mode == "swag"
    if mutation == "row stride D rounded up to 4":
        # the gradient pass is the right one (at stride D in the gradient buffer); the update takes row c of the state AND
        # of the gradients at c * D4 of the flat buffers and writes there; past the end of a buffer nothing exists
        D4 = 4 * ((D + 3) // 4)
        keys = ("theta", "mean", "sq") if swag else ("theta", "mean")
        flat = {key: np.concatenate([np.asarray(s0[key], dtype=dt).reshape(-1), np.zeros(P * D4 - P * D, dtype=dt)])
                for key in keys}
        grad_flat = np.zeros(P * D4, dtype=dt)
        losses = []
        for c in range(P):
            loss, g = sc._gradient(np.asarray(s0["theta"], dtype=dt)[c], data.step, case.step.spec, dt, None)
            grad_flat[c * D:(c + 1) * D] = g
            losses.append(loss)
        lr, n = dt(case.step.lr), dt(case.step.n0 + k)
        dev = np.asarray(s0["dev"], dtype=dt).copy() if swag else None
        for c in range(P):
            sl = slice(c * D4, c * D4 + D)
            th, mu, sq, dv = _update(mode, hit, col, flat["theta"][sl], grad_flat[sl], flat["mean"][sl],
                                     flat["sq"][sl] if swag else None, lr, n, dt)
            flat["theta"][sl], flat["mean"][sl] = th, mu
            if swag:
                flat["sq"][sl] = sq
                if dv is not None:
                    dev[c, col] = dv
        out = {key: flat[key][:P * D].reshape(P, D).copy() for key in keys}
        if swag:
            out["dev"] = dev
        out["loss"] = np.array(losses, dtype=dt)
        return out
    step_mut = {"count n + 1": "moments with count n + 1", "deviation against the old mean": "deviation against the old mean",
                "moments written on a non-hit step": "moments written on a non-update step"}.get(mutation)
    outs = []
    for c in range(P):
        o = sc.ref_step(case.step, data.step, mode, "plain", k, member_state(s0, c), dt, step_mut)
        if not swag:
            mean0 = np.asarray(s0["mean"], dtype=dt)[c]
            o["mean"] = o["theta"] if hit or mutation == "SGD mean copied on a miss step" else mean0
        outs.append(o)
    keys = ("theta", "mean", "sq", "dev") if swag else ("theta", "mean")
    out = {key: np.stack([np.asarray(o[key]) for o in outs]) for key in keys}
    out["loss"] = np.array([outs[0 if mutation == "member c's loss from member 0" else c]["loss"] for c in range(P)], dtype=dt)
    if mutation in ("member c's deviation written into member 0's block", "deviation column stride k D instead of D"):
        dev0 = np.asarray(s0["dev"], dtype=dt)
        flat = dev0.reshape(-1).copy()
        for c in range(P):
            if mutation == "member c's deviation written into member 0's block":
                at = col * D
            else:
                at = c * K_DEV * D + col * (K_DEV * D)
            if at + D <= flat.size:                    # (past the end of the buffer nothing exists for the caller)
                flat[at:at + D] = out["dev"][c, col]
        out["dev"] = flat.reshape(dev0.shape)
    return out


def as_stored(out: dict) -> dict:
    return {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}


# ---------------------------------------------------------------- the comparison
def compare_members_step(case, mode: str, k: int, s0: dict, got: dict, ref: dict, what: str = "") -> dict:
    """step_cases.compare_step for every member: row c of `got` against row c of the float64 reference `ref`, both from
    row c of s0.  SGD rows: the member's "mean" holds the bits of its stored new weights after a hit step, its old bits
    after a miss.  Raises AssertionError on the first bound a member misses; returns quantity -> the largest error over
    tolerance of any member."""
    rep = {}
    hit, _ = step_flags(mode, k)
    for c in range(case.P):
        w = f"{what}member {c} of {case.P}: "
        r = sc.compare_step(case.step, mode, k, member_state(s0, c), member_state(got, c), member_state(ref, c), what=w)
        for q, v in r.items():
            rep[q] = max(rep.get(q, 0.0), v)
        if mode == "sgd":
            want = got["theta"][c] if hit else s0["mean"][c]
            sc._same_bits(got["mean"][c], want, f"{w}{case.name} sgd step {k}: mean after a {'hit' if hit else 'miss'} step")
    return rep


# ---------------------------------------------------------------- the run
RUN_SIZES = cc.RUN_SIZES
run_lrs = cc.run_lrs
