"""Every eager SGD, SWAG, SGLD and BBB step path against the float64 oracle (tests/step_cases.py lists the cases and cells).

A test is one (case, mode): three consecutive steps on one plan, per noise variant of the mode.  Before every step the state
is read back and the reference restarts from it, so nothing accumulates and every bound is a bound on one step.  Per step:
the launches (k_wgrad_all<S> of the table on the fused path; k_dense_bwd_weight per layer and the mode's update kernel on the
other; k_bbb_sample for BBB), so a change in dispatch fails the case instead of quietly testing another kernel; then
step_cases.compare_step (increments per block, moments and deviation against the stored theta, losses); the sentinels
around every state buffer; that repeating the step from the same state gives the same bits; and, where the device draws the
noise, that the step with the same Philox stream injected gives the same bits."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import step_cases as sc  # noqa: E402
from dense_cases import ENV_FORBIDDEN  # noqa: E402
from step_cases import CASES, MODES, N_STEPS, STREAM, SWAG_STEPS, VARIANTS, compare_step, expected_step_launches, ref_step, step_data  # noqa: E402

SENTINEL = -12345.0
TAIL = 64
WORST = {}   # mode -> (largest error / tolerance, case, variant, quantity): printed at the end of the module


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in ENV_FORBIDDEN if os.environ.get(k)]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the library reads them once per process and every "
                    "expected launch of this module assumes their defaults -- unset them")
    from bayesian_inference_for_nn_amd import engine
    yield engine
    for mode, (ratio, name, variant, q) in sorted(WORST.items()):
        print(f"WORST | {mode} | error / tolerance {ratio:.4f} | {name} | {variant} | {q}")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Guarded:
    """A (D) float32 vector as a view into a sentinel-filled buffer: one element in front (the view then sits 4 bytes off
    16-byte alignment) or four (aligned), 64 behind."""

    def __init__(self, values, aligned):
        values = np.asarray(values, dtype=np.float32).reshape(-1)
        self.lead, self.D = (4 if aligned else 1), values.size
        self.buf = torch.full((self.lead + self.D + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.lead:self.lead + self.D]
        self.t.copy_(dev(values))
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (0 if aligned else 4) and self.t.is_contiguous()

    def set(self, values):
        self.t.copy_(dev(values))

    def get(self):
        return self.t.cpu().numpy().copy()

    def intact(self):
        return bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[self.lead + self.D:] == SENTINEL).all())


class Run:
    """The device side of one (case, mode): plan, data and guarded state buffers; `step` runs step k of a variant."""

    def __init__(self, eng, case, mode, data):
        self.eng, self.case, self.mode, self.data = eng, case, mode, data
        spec = case.spec
        self.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.max_batch)
        self.x = dev(data.x)
        self.y = dev(data.y, torch.int32 if spec.loss == "scce" else torch.float32)
        self.rid = dev(data.idx, torch.int32) if data.idx is not None else None
        s0 = sc.initial_state(mode, data)
        self.bufs = {}
        for key, v in s0.items():
            if key == "dev":
                for r in range(v.shape[0]):
                    self.bufs[f"dev{r}"] = Guarded(v[r], case.aligned)
            else:
                self.bufs[key] = Guarded(v, case.aligned)
        self.pm = Guarded(data.pm_vec, case.aligned) if case.prior_vec else None
        self.pr = Guarded(data.pr_vec, case.aligned) if case.prior_vec else None
        self.noise = Guarded(np.zeros(case.D), case.aligned)
        self.out = torch.zeros(4, device="cuda")

    def set_state(self, s):
        for key, v in s.items():
            if key == "dev":
                for r in range(v.shape[0]):
                    self.bufs[f"dev{r}"].set(v[r])
            else:
                self.bufs[key].set(v)

    def get_state(self):
        s = {key: b.get() for key, b in self.bufs.items() if not key.startswith("dev")}
        if self.mode == "swag":
            s["dev"] = np.stack([self.bufs["dev0"].get(), self.bufs["dev1"].get()])
        return s

    def guards_intact(self):
        return [key for key, b in list(self.bufs.items()) + [("noise", self.noise), ("pm", self.pm), ("pr", self.pr)]
                if b is not None and not b.intact()]

    def step(self, k, noise):
        """Step k with `noise` injected (a float32 vector, a device tensor, or None: the device draws it); returns the
        state after it with the loss (BBB: the cost triple) under "loss" / "cost"."""
        c, b, n = self.case, self.bufs, self.case.n0 + k
        kw = dict(batch=c.batch, row_idx=self.rid)
        z = None
        if noise is not None:
            self.noise.t.copy_(noise if isinstance(noise, torch.Tensor) else dev(noise))
            z = self.noise.t
        self.out.zero_()
        if self.mode == "sgd":
            self.plan.sgd_step(b["theta"].t, self.x, self.y, c.lr, self.out[:1], **kw)
        elif self.mode == "swag":
            update, row = SWAG_STEPS[k]
            self.plan.swag_step(b["theta"].t, b["mean"].t, b["sq"].t, None if row is None else b[f"dev{row}"].t, self.x, self.y,
                                c.lr, n, update, self.out[:1], **kw)
        elif self.mode == "sgld":
            self.plan.sgld_step(b["theta"].t, b["mean"].t, b["sq"].t, self.x, self.y, c.lr, n, c.seed, self.out[:1],
                                unit_noise=z, **kw)
        else:
            self.plan.bbb_step(b["mu"].t, b["rho"].t, b["w"].t, self.x, self.y, c.bbb_lr, c.alpha, c.prior[0], c.prior[1], n,
                               c.seed, self.out, eps=z, prior_mean_vec=self.pm.t if self.pm else None,
                               prior_rho_vec=self.pr.t if self.pr else None, **kw)
        got = self.get_state()
        o = self.out.cpu().numpy().copy()
        if self.mode == "bbb":
            got["cost"] = o[:3]
        else:
            got["loss"] = o[0]
        return got


def launched(kp):
    names = [n.replace(" ", "") for n, _ in kp.launches]
    return sc.StepLaunches(names.count(sc.SAMPLE_KERNEL),
                           tuple(n for n in names if "k_wgrad_all" in n or n.startswith("k_dense_bwd_weight")),
                           tuple(n for n in names if n in sc.UPDATE_KERNEL.values()), 0, "")


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k], dtype=np.float32).view(np.int32), np.asarray(b[k], dtype=np.float32).view(np.int32))
               for k in a)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_step_case(eng, case, mode):
    data = step_data(case)
    run = Run(eng, case, mode, data)
    exp = expected_step_launches(case, mode)
    worst = {}
    for variant in VARIANTS[mode]:
        run.set_state(sc.initial_state(mode, data))
        for k in range(N_STEPS):
            what = f"{case.name} {mode} {variant} step {k}"
            s0 = run.get_state()
            inj = sc.injected_noise(case, mode, variant, k) if mode in STREAM else None
            # 1. the launches
            with eng.KernelProbe(64) as kp:
                got = run.step(k, inj)
            la = launched(kp)
            assert (la.sample, la.wgrad, la.update) == (exp.sample, tuple(w.replace(" ", "") for w in exp.wgrad), exp.update), \
                (what, kp.launches, exp)
            # 2. - 4. increments, moments and deviation, losses against the float64 reference restarted from s0
            ref = ref_step(case, data, mode, variant, k, s0)
            rep = compare_step(case, mode, k, s0, got, ref, what=f"{variant}: ")
            for q, r in sorted(rep.items()):
                print(f"{what}: {q}: error / tolerance {r:.4f}")
                worst[q] = max(worst.get(q, 0.0), r)
                if r > WORST.get(mode, (-1.0,))[0]:
                    WORST[mode] = (r, case.name, variant, q)
            # 6. the sentinels around every buffer
            assert run.guards_intact() == [], f"{what}: wrote outside {run.guards_intact()}"
            # 7. the same step from the same state: the same bits
            run.set_state(s0)
            again = run.step(k, inj)
            assert same_bits(got, again), f"{what}: repeating the step from the same state gives other bits"
            # 5. the device's own draws are the Philox stream fill_normal writes, element by element
            if variant == "device":
                z = eng.fill_normal(torch.empty(case.D, device="cuda"), case.seed, STREAM[mode], case.n0 + k)
                run.set_state(s0)
                injected = run.step(k, z)
                assert same_bits(got, injected), f"{what}: device noise and the injected stream give different bits"
            assert run.guards_intact() == [], f"{what}: wrote outside {run.guards_intact()}"
    print(f"CASE | {case.name} | {mode} | " + " | ".join(f"{q} {r:.4f}" for q, r in sorted(worst.items())))
    run.plan.close()


FINITE_CASES = {"fused": "f_s1", "unfused": "u_d99"}


@pytest.mark.parametrize("path", ["fused", "unfused"])
@pytest.mark.parametrize("mode", MODES)
def test_check_finite_sees_a_diverged_step(eng, mode, path):
    """include/pyz.h: every kernel that finalises a step's loss counts NaN / Inf results for pyz_check_finite.  A NaN in
    the last layer's last bias reaches the loss whatever the activations are."""
    from bayesian_inference_for_nn_amd._lib import E_NAN, PyzError
    case = sc.CASE_BY_NAME[FINITE_CASES[path]]
    assert case.fused == (path == "fused")
    data = step_data(case)
    run = Run(eng, case, mode, data)
    noise = sc.injected_noise(case, mode, "philox", 0) if mode in STREAM else None
    got = run.step(0, noise)
    assert np.all(np.isfinite(got["cost"] if mode == "bbb" else got["loss"]))
    run.plan.check_finite()
    s = sc.initial_state(mode, data)
    s["mu" if mode == "bbb" else "theta"][case.D - 1] = np.nan
    run.set_state(s)
    got = run.step(0, noise)
    assert np.isnan(got["cost"][0] if mode == "bbb" else got["loss"])
    with pytest.raises(PyzError) as e:
        run.plan.check_finite()
    assert e.value.code == E_NAN
    run.plan.check_finite()      # the count was reset
    run.plan.close()
