"""Every SVGD kernel path through its squared distances, its kernel rows and phi, against float64 arithmetic on the float32
inputs (tests/svgd_cases.py lists the cases and cells).

A test is one case: Adam's first step from a zero state, which leaves phi itself in m (observable (b): repulsion only,
drive only or both, each on its own scale; v in units of its last place; the step's loss, (d)), and on the coupled cases one
step at t = 7 from a non-zero Adam state ((c): m, v and the particles with phi's tolerance carried through Adam).  Per
call: the launches under KernelProbe against the table, so a change in dispatch fails the case instead of quietly testing
another kernel; the sentinels around particles, snapshot, m, v and loss; the snapshot unchanged by a Jacobi call; the same
call from the same state giving the same bits.  The squared distances themselves ((a)) are read through
pyz_svgd_gram_groups in both forms.  Under Gauss-Seidel the reference of row i is evaluated against the rows the device
stored before it: every bound is a bound on one row, and a row that did not see its predecessors misses it."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import svgd_cases as sv  # noqa: E402
from dense_cases import ENV_FORBIDDEN  # noqa: E402
from svgd_cases import CASES, DIST_CASES, compare_adam, compare_distances, compare_phi, expected_svgd_launches, svgd_data  # noqa: E402

SENTINEL = -12345.0
TAIL = 64
UNWRITTEN = 777.0        # what the rows a Jacobi call only writes hold before it
WORST = {}               # observable -> (largest error / tolerance, case): printed at the end of the module


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in ENV_FORBIDDEN + (sv.ENV_NEVER,) + tuple(sv.ENV_DEFAULTS) if os.environ.get(k)]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: every expected launch of this module assumes the defaults "
                    "and sets the per-call switches itself -- unset them")
    from bayesian_inference_for_nn_amd import engine
    yield engine
    for q, (ratio, name) in sorted(WORST.items()):
        print(f"WORST | {q} | error / tolerance {ratio:.4f} | {name}")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Guarded:
    """A (rows, D) matrix as a view into a sentinel-filled buffer: four elements in front (16-byte aligned) or one (the
    view then sits one element off 16-byte alignment), 64 behind."""

    def __init__(self, values, aligned=True, dtype=torch.float32):
        values = np.asarray(values)
        self.shape, n = values.shape, values.size
        self.lead = 4 if aligned else 1
        self.buf = torch.full((self.lead + n + TAIL,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[self.lead:self.lead + n].view(*self.shape)
        self.n = n
        self.set(values)
        esz = self.buf.element_size()
        assert self.buf.data_ptr() % 16 == 0 and self.t.is_contiguous()
        assert self.t.data_ptr() % 16 == (0 if aligned else esz) and (dtype != torch.float32 or aligned or self.t.data_ptr() % 16 == 4)

    def set(self, values):
        self.t.copy_(dev(values, self.buf.dtype).view(*self.shape))

    def get(self):
        return self.t.cpu().numpy().copy()

    def intact(self):
        return bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[self.lead + self.n:] == SENTINEL).all())


def set_switches(monkeypatch, env):
    for k in sv.ENV_DEFAULTS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, str(v))


class Run:
    """The device side of one case: plan, data and guarded buffers; `step` runs one pyz_svgd_step from a given state."""

    def __init__(self, eng, case, data):
        self.eng, self.case, self.data = eng, case, data
        spec = case.spec
        self.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.batch, max_particles=case.nl)
        self.x = dev(data.x)
        self.y = dev(data.y, torch.int32 if spec.loss == "scce" else torch.float32)
        zero = np.zeros((case.nl, case.D), dtype=np.float32)
        if case.sweep == "gs":
            self.local = self.snap = Guarded(data.parts)
        else:
            self.snap = Guarded(data.parts, aligned=not case.snap_off)
            self.local = Guarded(np.full_like(zero, UNWRITTEN))
        self.m, self.v, self.loss = Guarded(zero), Guarded(zero), Guarded(np.zeros((1, 1), dtype=np.float32))
        self.bufs = {"particles": self.local, "snapshot": self.snap, "m": self.m, "v": self.v, "loss": self.loss}

    def guards(self):
        return [k for k, b in self.bufs.items() if not b.intact()]

    def step(self, m0, v0, t):
        c = self.case
        self.snap.set(self.data.parts)
        if c.sweep == "jacobi":
            self.local.set(np.full(self.local.shape, UNWRITTEN, dtype=np.float32))
        self.m.set(m0)
        self.v.set(v0)
        self.loss.set(np.full((1, 1), UNWRITTEN, dtype=np.float32))
        self.plan.svgd_step(self.local.t, self.snap.t, c.row0, self.m.t, self.v.t, self.x, self.y, sv.LR, c.gamma, t,
                            self.loss.t.view(1), sweep="gauss_seidel" if c.sweep == "gs" else "jacobi")
        torch.cuda.synchronize()
        got = {"m": self.m.get(), "v": self.v.get(), "x": self.local.get(), "loss": float(self.loss.get()[0, 0])}
        if c.sweep == "jacobi":
            assert np.array_equal(self.snap.get().view(np.int32), self.data.parts.view(np.int32)), f"{c.name}: a Jacobi call changed its snapshot"
        return got


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k], dtype=np.float32).view(np.int32), np.asarray(b[k], dtype=np.float32).view(np.int32))
               for k in a)


def note(rep, case, prefix):
    for q, r in sorted(rep.items()):
        print(f"{case.name}: {prefix} {q}: error / tolerance {r:.4f}")
        if r > WORST.get(f"{prefix} {q}", (-1.0,))[0]:
            WORST[f"{prefix} {q}"] = (r, case.name)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_svgd_case(eng, monkeypatch, case):
    data = svgd_data(case)
    set_switches(monkeypatch, case.env)
    run = Run(eng, case, data)
    exp = expected_svgd_launches(case, torch.cuda.get_device_properties(0).multi_processor_count)
    zero = np.zeros((case.nl, case.D), dtype=np.float32)
    steps = [("(b)", zero, zero, 1, compare_phi)]
    if sv.has_adam_step(case):
        steps.append(("(c)", data.m0, data.v0, sv.T_ADAM, compare_adam))
    for label, m0, v0, t, compare in steps:
        what = f"{case.name} {label} t={t}"
        # 1. the launches
        with eng.KernelProbe(512) as kp:
            got = run.step(m0, v0, t)
        assert sv.svgd_kernels(kp.launches) == exp, (what, sv.svgd_kernels(kp.launches), exp)
        # a resident sweep that could not meet leaves a NaN loss and the plan's count: a finding, not a case
        assert np.isfinite(got["loss"]), f"{what}: loss {got['loss']!r}"
        run.plan.check_finite()
        assert not np.any(got["x"] == UNWRITTEN), f"{what}: rows of the output were not written"
        # 2. the observables against the float64 reference
        note(compare(case, data, got), case, label)
        # 3. the sentinels around every buffer
        assert run.guards() == [], f"{what}: wrote outside {run.guards()}"
        # 4. the same call from the same state: the same bits (the large models run one step)
        if not case.big:
            again = run.step(m0, v0, t)
            assert same_bits(got, again), f"{what}: repeating the call from the same state gives other bits"
            assert run.guards() == [], f"{what}: wrote outside {run.guards()}"
    run.plan.close()


@pytest.mark.parametrize("gram", [1, 0], ids=["gram", "pairwise"])
@pytest.mark.parametrize("name", DIST_CASES)
def test_squared_distances(eng, monkeypatch, name, gram):
    """Observable (a): the eight (64, 64) float64 group tiles of pyz_svgd_gram_groups, summed in float64 on the host, are the
    device's squared distances."""
    case = sv.CASE_BY_NAME[name]
    parts = sv.dist_parts(case)
    M, D = case.M, case.D
    set_switches(monkeypatch, {"PYZ_SVGD_GRAM": gram})
    spec = case.spec
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.batch, max_particles=M)
    snap = Guarded(parts)
    fill = np.full((sv.GROUPS, 4096), UNWRITTEN)
    groups = Guarded(fill, dtype=torch.float64)

    def call(ranges):
        groups.set(fill)
        for lo, hi in ranges:
            with eng.KernelProbe(16) as kp:
                plan.svgd_gram_groups(snap.t, lo, hi, groups.t)
            assert sv.svgd_kernels(kp.launches) == sv.expected_group_launches(M, D, lo, hi, bool(gram)), (name, lo, hi, kp.launches)
        torch.cuda.synchronize()
        assert snap.intact() and groups.intact(), f"{name}: wrote outside the snapshot or the group buffer"
        assert np.array_equal(snap.get().view(np.int32), parts.view(np.int32))
        return groups.get().reshape(sv.GROUPS, 64, 64)

    whole = call([(0, sv.GROUPS)])
    assert not np.any(whole[:, :M, :M] == UNWRITTEN)
    d2 = whole.sum(axis=0)[:M, :M]
    note(compare_distances(parts, d2, "gram" if gram else "pairwise", what=name), case, "(a)")
    split = call([(0, 3), (3, sv.GROUPS)])
    assert np.array_equal(whole.view(np.int64), split.view(np.int64)), f"{name}: groups [0, 3) then [3, 8) differ from [0, 8)"
    again = call([(0, sv.GROUPS)])
    assert np.array_equal(whole.view(np.int64), again.view(np.int64)), f"{name}: repeating the call gives other bits"
    plan.close()


def test_jacobi_in_place_is_refused(eng, monkeypatch):
    """A Jacobi sweep whose output rows lie inside its snapshot would read rows other workgroups of the same launch write:
    PYZ_E_INVALID before anything is enqueued -- particles, m and v unchanged, no launch under the probe.  (The refused
    call is the whole test: the race itself is never run.)"""
    from bayesian_inference_for_nn_amd._lib import PyzError
    E_INVALID = -1      # PYZ_E_INVALID of include/pyz.h
    case = sv.CASE_BY_NAME["j_rows_a1_m5"]
    data = svgd_data(case)
    set_switches(monkeypatch, {})
    spec, M, D = case.spec, case.M, case.D
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.batch, max_particles=M)
    x, y = dev(data.x), dev(data.y, torch.int32)
    P = Guarded(data.parts)
    state = np.full((M, D), 0.25, dtype=np.float32)
    m, v, loss = Guarded(state), Guarded(state), torch.full((1,), UNWRITTEN, device="cuda")
    calls = [lambda: plan.svgd_step(P.t, P.t, 0, m.t, v.t, x, y, sv.LR, 0.37, 1, loss, sweep="jacobi"),          # the same buffer
             lambda: plan.svgd_step(P.t[2:4], P.t, 2, m.t[2:4], v.t[2:4], x, y, sv.LR, 0.37, 1, loss, sweep="jacobi"),   # rows inside it
             lambda: plan.svgd_sweep(P.t, P.t, 0, m.t, v.t, sv.LR, 0.37, 1, loss, sweep="jacobi")]
    for call in calls:
        with eng.KernelProbe(64) as kp:
            with pytest.raises(PyzError) as e:
                call()
        assert e.value.code == E_INVALID and kp.launches == []
    torch.cuda.synchronize()
    assert np.array_equal(P.get(), data.parts) and np.array_equal(m.get(), state) and np.array_equal(v.get(), state)
    assert float(loss) == UNWRITTEN and P.intact() and m.intact() and v.intact()
    # the Gauss-Seidel sweep in place and a Jacobi sweep on a separate snapshot go on as before
    plan.svgd_step(P.t, P.t, 0, m.t, v.t, x, y, sv.LR, 0.37, 1, loss, sweep="gauss_seidel")
    plan.svgd_step(P.t, dev(data.parts), 0, m.t, v.t, x, y, sv.LR, 0.37, 1, loss, sweep="jacobi")
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    plan.check_finite()
    plan.close()
