"""Every FSVI step path on the device against the restatement (tests/fsvi_cases.py lists the cases and cells), on inputs
whose GP prior matrix is not the identity.

A test is one case: two chained steps (t = 1, 2) with injected draws on one plan.  Before every step the stored state is read
back and the reference restarts from it, so every bound is a bound on one step.  Per step: the launches (the solve variant of
both systems, the forward kernel of every layer: a change in dispatch fails the case instead of quietly testing another
kernel); the window of cond(K_i) and of the off-diagonal entries, from the Xp the device assembled; fsvi_cases.compare_step
(xp and the redraw bit for bit, alpha, c2, f, g per layer block, the loss, the Adam update); and that the step repeated from
the same state gives the same bits.  Then: the Philox draws at sizes past one 256-thread stripe, the growth of the plan's
FSVI workspace between calls, the non-positive-pivot arm inside a step.  The solver alone at its remaining sizes is in
tests/test_gpu_fsvi.py."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fsvi_cases as fv  # noqa: E402
import fsvi_checks as fc  # noqa: E402
from dense_cases import ENV_FORBIDDEN  # noqa: E402
from fsvi_cases import CASES, LR, N_STEPS, SEED, case_data, compare_step, expected_fsvi_launches  # noqa: E402

from bayesian_inference_for_nn_amd import _lib  # noqa: E402

PER_CALL_ENV = ("PYZ_FWD_LDS", "PYZ_FWD_LDS_MINWG")
KEYS = ("xp", "f", "alpha", "c2", "g", "loss", "mu", "m", "v", "W")
WORST = {}       # quantity -> (largest error / tolerance, case, step): printed at the end of the module
SEEN = set()     # kernel expressions the probes of this module reported
RAN = set()


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in ENV_FORBIDDEN if os.environ.get(k)]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the library reads them once per process and every "
                    "expected launch of this module assumes their defaults -- unset them")
    from bayesian_inference_for_nn_amd import engine
    yield engine
    for q, (ratio, name, t) in sorted(WORST.items()):
        print(f"WORST | {q} | error / tolerance {ratio:.4f} | {name} | t={t}")


@pytest.fixture(autouse=True)
def per_call_switches(monkeypatch):
    for k in PER_CALL_ENV:
        monkeypatch.delenv(k, raising=False)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy().copy()


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[q]).view(np.uint8), np.asarray(b[q]).view(np.uint8)) for q in a)


class Run:
    """A plan, the device state of one FSVI run of a case, and its data."""

    def __init__(self, eng, case, plan=None, state=None):
        self.eng, self.case, self.data = eng, case, case_data(case)
        spec = case.spec
        self.plan = plan or eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, "mse"), max_batch=case.max_batch, max_particles=case.k)
        self.x, self.y = dev(self.data.x), dev(self.data.y)
        rows = self.data.x[np.abs(self.data.x).max(axis=1) < fv.FAR / 10]
        self.lo, self.hi = dev(rows.min(axis=0)), dev(rows.max(axis=0))
        self.bufs = {q: dev(v) for q, v in (state or fv.initial_state(self.data)).items()}
        self.loss = torch.zeros(1, device="cuda")
        self.launches = None

    def set_state(self, s):
        for q, v in s.items():
            self.bufs[q].copy_(dev(v))

    def get_state(self):
        return {q: host(b) for q, b in self.bufs.items()}

    def step(self, t, draws=None, idx=None, seed=SEED, probe=False, lo=None, hi=None):
        """Step t with the Draws injected (None: the device draws; idx then names the batch rows)."""
        c, b = self.case, self.bufs
        idx = draws.idx if draws is not None else idx
        inj = dict(xm=dev(draws.xm), noise=dev(draws.z), eps=dev(draws.eps)) if draws is not None else {}
        self.loss.zero_()
        call = lambda: self.plan.fsvi_step(b["mu"], b["W"], b["m"], b["v"], self.x, self.y, c.B, LR, t, seed, self.loss,
                                           lo=self.lo if lo is None else lo, hi=self.hi if hi is None else hi, want_terms=True,
                                           batch=c.b, row_idx=None if idx is None else dev(idx, torch.int32), **inj)
        if probe:
            with self.eng.KernelProbe(64) as kp:
                got = call()
            names = tuple(n.replace(" ", "") for n, _ in kp.launches)
            SEEN.update(names)
            self.launches = tuple(n for n in names if n.startswith(fv.WATCHED))
        else:
            got = call()
        out = {"xp": host(got["xp"]), "f": host(got["f"]), "alpha": host(got["alpha"]), "c2": host(got["stein"]),
               "g": host(got["grad"]), "loss": host(self.loss)}
        out.update(self.get_state())
        return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_fsvi_case(eng, case, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    run = Run(eng, case)
    exp = expected_fsvi_launches(case)
    worst = {}
    for t in range(1, N_STEPS + 1):
        what = f"{case.name} t={t}"
        d = run.data.steps[t - 1]
        s0 = run.get_state()
        got = run.step(t, d, probe=True)
        # 1. the launches
        print(f"{what}: launches " + " ".join(run.launches))
        assert run.launches == tuple(n.replace(" ", "") for n in exp.sequence), (what, run.launches, exp.sequence)
        # 2. the GP prior matrix of every particle is not the identity, from the device's own Xp
        conds = fv.assert_input_conditions(got["xp"], what)
        print(f"{what}: cond(K_i) " + " ".join(f"{c:.2f}" for c, _ in conds) + ", median row maximum " +
              " ".join(f"{m:.3f}" for _, m in conds))
        # 3. every term, the gradient per layer block and the update against the reference restarted from s0
        rep = compare_step(case, run.data, t, s0, got, what="device: ")
        for q, r in sorted(rep.items()):
            print(f"{what}: {q}: error / tolerance {r:.4f}")
            worst[q] = max(worst.get(q, 0.0), r)
            if r > WORST.get(q, (-1.0,))[0]:
                WORST[q] = (r, case.name, t)
        # 4. the same step from the same state: the same bits
        after = run.get_state()
        run.set_state(s0)
        again = run.step(t, d)
        assert same_bits(got, again), f"{what}: repeating the step from the same state gives other bits"
        assert same_bits(after, run.get_state())
    run.plan.check_finite()
    print(f"CASE | {case.name} | " + " | ".join(f"{q} {r:.4f}" for q, r in sorted(worst.items())))
    RAN.add(case.name)
    run.plan.close()


def test_every_kernel_of_the_table_was_launched(eng):
    if len(RAN) < len(CASES):
        return      # a selection of cases was run: nothing to conclude
    want = {"k_fsvi_inputs", "k_fsvi_stein_system", "k_fsvi_gram", "k_fsvi_delta", "k_fsvi_update", "k_spd_solve_f64<true>",
            "k_spd_solve_f64<false>", "k_dense_fwd", "k_dense_fwd_lds<2>", "k_dense_bwd_data", "k_dense_bwd_weight"}
    assert want <= SEEN, sorted(want - SEEN)


# ---------------------------------------------------------------- the Philox draws past one stripe
@pytest.mark.parametrize("name", ["d385", "rows514"])
def test_philox_draws_are_the_oracle_stream(eng, name):
    """No injected draws: the step equals the step fed with fsvi_checks.draw_* (the comparison of
    tests/test_gpu_fsvi.py::test_philox_draws_are_the_oracle_stream, at k D = 770 and B F = 514 elements: more than one
    Philox counter per thread stripe, and element indices past 256).  The measurement rows are drawn in a box of +-3000 per
    feature, so that they lie far apart and far from the batch rows: the device's float32 Box-Muller differs from the
    oracle's by up to 3.2e-5 per normal, an Xp entry may round the other way, and a K_i with two rows close together would
    amplify that, which is not what this measures.  (The batch rows keep their lattice.)"""
    assert _lib.STREAM_FSVI == fc.STREAM == 9
    case = fv.CASE_BY_NAME[name]
    t, seed = 6, 4242
    data = case_data(case)
    idx = data.steps[0].idx
    lo, hi = np.full(case.F, -3000.0, np.float32), np.full(case.F, 3000.0, np.float32)

    def one(t, injected):
        run = Run(eng, case)
        draws = None
        if injected:
            draws = fv.Draws(idx, fc.draw_xm(seed, t, case.B, case.F, lo, hi), fc.draw_noise(seed, t, case.k, case.F),
                             fc.draw_eps(seed, t, case.k, case.D))
        got = run.step(t, draws, idx=idx, seed=seed, lo=dev(lo), hi=dev(hi))
        run.plan.check_finite()
        run.plan.close()
        return {q: got[q] for q in ("xp", "g", "mu", "W", "loss")}

    own, inj = one(t, False), one(t, True)
    for q in own:
        r = fv._close(own[q], inj[q], 1e-4, f"{name}: Philox against injected oracle draws: {q}")
        print(f"{name}: Philox against injected oracle draws: {q}: error / tolerance {r:.4f}")
    # xp at 1e-4 of 3000 says little: the batch rows differ by the Box-Muller difference of z_i (0.1 x 3.2e-5) and one
    # float32 rounding of x + z at |x| < 32 (1.9e-6 each side); the measurement rows, X_M restated bit for bit, by one
    # rounding at 3000 (2^-12) each side
    batch_err = np.abs(own["xp"][:, :case.b] - inj["xp"][:, :case.b]).max()
    meas_err = np.abs(own["xp"][:, case.b:] - inj["xp"][:, case.b:]).max()
    print(f"{name}: Philox against injected oracle draws: xp batch rows {batch_err:.3e}, measurement rows {meas_err:.3e}")
    assert np.abs(inj["xp"][:, :case.b]).max() < 32.0 and batch_err <= 3.2e-6 + 2 * 1.91e-6 and meas_err <= 2.0 ** -11
    assert same_bits(own, one(t, False)), "same (seed, t): same step"
    other = one(t + 1, False)
    assert np.abs(other["xp"] - own["xp"]).max() > 1.0 and np.abs(other["W"] - own["W"]).max() > 0.1


# ---------------------------------------------------------------- growth of the plan's FSVI workspace
def test_workspace_grows_between_calls_and_keeps_the_results(eng):
    """One plan runs k = 1, b = B = 5, then k = 3, b = B = 64 (Xp, both float64 systems and the gradient rows all need
    more), then the first call again; each result equals that call on a fresh plan bit for bit, and the workspace grew once."""
    dims, acts = (2, 40, 1), ("relu", "linear")
    small, large = fv.FsviCase("grow_small", dims, acts, 1, 5, 5), fv.FsviCase("grow_large", dims, acts, 3, 64, 64)
    spec = small.spec

    def new_plan():
        return eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, "mse"), max_batch=large.max_batch, max_particles=large.k)

    def call(plan, case):
        run = Run(eng, case, plan=plan)
        got = run.step(1, run.data.steps[0])
        plan.check_finite()
        return got

    plan = new_plan()
    sizes, got = [plan.workspace_bytes], []
    for case in (small, large, small):
        got.append(call(plan, case))
        sizes.append(plan.workspace_bytes)
    print("workspace bytes:", sizes)
    assert sizes[0] < sizes[1] < sizes[2] == sizes[3], sizes
    for case, g in zip((small, large, small), got):
        fresh = new_plan()
        want = call(fresh, case)
        fresh.close()
        assert same_bits(g, want), f"{case.name}: the result on the grown plan differs from a fresh plan's"
    assert same_bits(got[0], got[2])
    data = case_data(large)      # and the large call is right, not only repeatable
    compare_step(large, data, 1, fv.initial_state(data), got[1], what="grown plan: ")
    plan.close()


# ---------------------------------------------------------------- the non-positive-pivot arm of a step
def test_a_nan_weight_takes_the_pivot_arm(eng):
    """Deviation 5 of A8 inside a step: one particle of `d161` holds a NaN weight (the last layer's bias: whatever the
    hidden activation makes of a NaN, f is NaN), so its Stein matrix has no positive pivot at that column (the global path,
    D = 161: the last panel, of one column).  The call returns normally, the loss is NaN and the plan's sentinel counts it
    as it would any NaN loss; the other particles' alpha and c2 still match."""
    case = fv.CASE_BY_NAME["d161"]
    data = case_data(case)
    s0 = fv.initial_state(data)
    bad, col = 1, case.D - 1
    s0["W"][bad, col] = np.nan
    run = Run(eng, case, state=s0)
    d = data.steps[0]
    got = run.step(1, d)
    torch.cuda.synchronize()
    assert np.isnan(got["loss"]).all()
    with pytest.raises(_lib.PyzError) as e:
        run.plan.check_finite()
    assert e.value.code == _lib.E_NAN
    run.plan.check_finite()      # (the count was reset)
    assert np.isnan(got["c2"][bad]).all() and np.isnan(got["alpha"][bad]).all()
    xd, _ = fv.batch_of(case, data, d)
    xp = fc.make_xp(xd, d.xm, d.z)
    assert np.array_equal(got["xp"], xp)
    for i in (0, 2):
        r = fv._close(got["alpha"][i], fc.gp_alpha(fc.gram(xp[i]), got["f"][i].astype(np.float64)), fv.REL_ALPHA, f"alpha of particle {i}")
        r2 = fv._close(got["c2"][i], fc.stein_c2(s0["W"][i]).astype(np.float32), fv.REL_C2, f"c2 of particle {i}")
        print(f"pivot arm: particle {i}: alpha error / tolerance {r:.4f}, c2 {r2:.4f}")
    run.plan.close()
