"""SGLD lanes on the device: pyz_sgld_lanes_step against the float64 restatement (tests/sgld_lanes_checks.py lists the cases),
what it shares bit for bit with pyz_sgld_chains_step, no cross-talk between the lanes' rates, the shared noise stream, and
pyz_sgld_lanes_run against the step calls bit for bit.

A step test is one case: per seed stride and noise variant three consecutive steps from n0 = 3.  Before every step the
state is read back and the reference restarts from it, so every bound is step_cases.compare_step's bound on one step of one
chain.  Every buffer the kernels write sits between sentinels, and the sentinels stay."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bce_checks  # noqa: E402
import sgld_lanes_checks as lc  # noqa: E402

SENTINEL = -12345.0
TAIL = 64


@pytest.fixture(scope="module")
def eng(gpu_device):
    from bayesian_inference_for_nn_amd import engine
    return engine


@pytest.fixture(autouse=True)
def bce(monkeypatch):
    bce_checks.install(monkeypatch)          # the oracle restated for the BCE case of the list


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


class Guarded:
    """A float32 array as a view into a sentinel-filled buffer: one element in front (the array then starts 4 bytes off
    16-byte alignment) or four (aligned), 64 behind."""

    def __init__(self, values, aligned):
        values = np.asarray(values, dtype=np.float32)
        self.lead, self.shape = (4 if aligned else 1), values.shape
        n = values.size
        self.buf = torch.full((self.lead + n + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.lead:self.lead + n].view(*self.shape)
        self.t.copy_(dev(values))
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (0 if aligned else 4) and self.t.is_contiguous()

    def set(self, values):
        self.t.copy_(dev(values))

    def get(self):
        return self.t.cpu().numpy().copy()

    def intact(self):
        n = int(np.prod(self.shape))
        return bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[self.lead + n:] == SENTINEL).all())


class Run:
    """The device side of one case: a plan for P particles, the data and guarded (P, D) state buffers."""

    def __init__(self, eng, case, data):
        self.case, st = case, case.step
        self.P = case.P
        spec = st.spec
        self.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=st.max_batch, max_particles=case.P)
        self.x = dev(data.step.x)
        self.y = dev(data.step.y, torch.int32 if spec.loss == "scce" else torch.float32)
        self.rid = dev(data.step.idx, torch.int32) if data.step.idx is not None else None
        zero = np.zeros((self.P, case.D))
        self.bufs = {k: Guarded(zero, st.aligned) for k in ("theta", "mean", "sq")}
        self.noise = Guarded(zero, st.aligned)
        self.loss = Guarded(np.zeros(self.P), True)

    def set_state(self, s):
        for k, b in self.bufs.items():
            b.set(s[k])

    def get_state(self):
        return {k: b.get() for k, b in self.bufs.items()}

    def guards_broken(self):
        return [k for k, b in list(self.bufs.items()) + [("noise", self.noise), ("loss", self.loss)] if not b.intact()]

    def _noise(self, noise):
        if noise is None:
            return None
        self.noise.t.copy_(noise if isinstance(noise, torch.Tensor) else dev(noise))
        return self.noise.t

    def _result(self):
        got = self.get_state()
        got["loss"] = self.loss.get()
        return got

    def step(self, k, noise, rates, stride):
        st, b = self.case.step, self.bufs
        z = self._noise(noise)
        self.loss.t.zero_()
        self.plan.sgld_lanes_step(b["theta"].t, b["mean"].t, b["sq"].t, self.x, self.y, rates, st.n0 + k, st.seed, self.loss.t,
                                  seed_stride=stride, batch=st.batch, row_idx=self.rid, unit_noise=z)
        return self._result()

    def chains_step(self, k, noise):
        st, b = self.case.step, self.bufs
        z = self._noise(noise)
        self.loss.t.zero_()
        self.plan.sgld_chains_step(b["theta"].t, b["mean"].t, b["sq"].t, self.x, self.y, st.lr, st.n0 + k, st.seed, self.loss.t,
                                   batch=st.batch, row_idx=self.rid, unit_noise=z)
        return self._result()


@pytest.mark.parametrize("case", lc.CASES, ids=[c.name for c in lc.CASES])
def test_step_case(eng, case):
    data = lc.chains_data(case)
    run = Run(eng, case, data)
    rates = lc.lane_rates(case)
    worst = {}
    for stride in lc.STRIDES:
        for variant in lc.VARIANTS:
            run.set_state(lc.initial_state(data))
            for k in range(lc.N_STEPS):
                what = f"{case.name} stride {stride} {variant} step {k}"
                s0 = run.get_state()
                got = run.step(k, lc.injected_noise(case, variant, k, stride), rates, stride)
                ref = lc.ref_lanes_step(case, data, variant, k, s0, stride)
                rep = lc.compare_lanes_step(case, k, s0, got, ref, stride, what=f"stride {stride} {variant}: ")
                for q, r in sorted(rep.items()):
                    print(f"{what}: {q}: error / tolerance {r:.4f}")
                    worst[q] = max(worst.get(q, 0.0), r)
                assert run.guards_broken() == [], f"{what}: wrote outside {run.guards_broken()}"
    print(f"CASE | {case.name} | " + " | ".join(f"{q} {r:.4f}" for q, r in sorted(worst.items())))
    run.plan.close()


@pytest.mark.parametrize("case", lc.CASES, ids=[c.name for c in lc.CASES])
def test_equal_rates_and_stride_one_are_the_chains_step_bit_for_bit(eng, case):
    data = lc.chains_data(case)
    s0 = lc.initial_state(data)
    run = Run(eng, case, data)
    rates = np.full(case.P, case.step.lr, dtype=np.float32)
    for variant in ("philox", "device"):
        inj = lc.injected_noise(case, variant, 1, 1)
        run.set_state(s0)
        chains = run.chains_step(1, inj)
        run.set_state(s0)
        lanes = run.step(1, inj, rates, 1)
        for key in ("theta", "mean", "sq", "loss"):
            assert np.array_equal(bits(lanes[key]), bits(chains[key])), f"{case.name} {variant}: {key} differs from sgld_chains_step"
        # the same step from the same state: the same bits
        run.set_state(s0)
        assert same_bits(lanes, run.step(1, inj, rates, 1)), f"{case.name} {variant}: repeating the step gives other bits"
    assert run.guards_broken() == []
    run.plan.close()


CROSS_TALK = ("f_d66_gathered_p5", "u_d165_mse_p5")


@pytest.mark.parametrize("name", CROSS_TALK)
def test_a_lane_keeps_its_bits_when_the_other_rates_change(eng, name):
    case = lc.CASE_BY_NAME[name]
    data = lc.chains_data(case)
    s0 = lc.initial_state(data)
    run = Run(eng, case, data)
    rates = lc.lane_rates(case)
    for stride in lc.STRIDES:
        for variant in ("philox", "device"):
            inj = lc.injected_noise(case, variant, 1, stride)
            run.set_state(s0)
            got = run.step(1, inj, rates, stride)
            for c in range(case.P):
                other = (rates[::-1] * np.float32(0.375)).astype(np.float32)
                other[c] = rates[c]
                assert all(other[j] != rates[j] for j in range(case.P) if j != c)
                run.set_state(s0)
                again = run.step(1, inj, other, stride)
                for key in ("theta", "mean", "sq", "loss"):
                    assert np.array_equal(bits(again[key][c]), bits(got[key][c])), \
                        f"{name} stride {stride} {variant}: row {c} of {key} moved with the other lanes' rates"
                moved = [j for j in range(case.P) if j != c and not np.array_equal(bits(again["theta"][j]), bits(got["theta"][j]))]
                assert moved == [j for j in range(case.P) if j != c], "the other lanes did take their new rates"
    assert run.guards_broken() == []
    run.plan.close()


@pytest.mark.parametrize("name", ("f_d404_p5", "u_d1100_p5", "f_d25_odd_p2"))
def test_shared_stream_equal_start_and_equal_rate_give_equal_rows(eng, name):
    """Stride 0: rows 0 and P - 1 start equal and step with the same rate, the rows between with others.  The two come out
    equal bit for bit (same batch, same gradient arithmetic per row, ONE noise stream); with stride 1 they do not."""
    case = lc.CASE_BY_NAME[name]
    data = lc.chains_data(case)
    s0 = lc.initial_state(data)
    last = case.P - 1
    for key in s0:
        s0[key][last] = s0[key][0]
    rates = lc.lane_rates(case)
    rates[last] = rates[0]
    run = Run(eng, case, data)
    for stride in (0, 1):
        run.set_state(s0)
        for k in range(2):
            got = run.step(k, None, rates, stride)
        equal = all(np.array_equal(bits(got[key][0]), bits(got[key][last])) for key in ("theta", "mean", "sq", "loss"))
        assert equal == (stride == 0), f"{name} stride {stride}: rows 0 and {last} {'differ' if stride == 0 else 'are equal'}"
        if case.P > 2:
            assert not np.array_equal(bits(got["theta"][0]), bits(got["theta"][1]))
    assert run.guards_broken() == []
    run.plan.close()


# ---------------------------------------------------------------- the run
RUN_SHAPES = {
    "fused_p3": ((5, 7, 3), ("tanh", "softmax"), "scce", 3),
    "unfused_p2": ((3, 5, 33), ("tanh", "softmax"), "scce", 2),
}


@pytest.mark.parametrize("shape", sorted(RUN_SHAPES))
@pytest.mark.parametrize("stride", lc.STRIDES)
def test_run_equals_step_calls_bit_for_bit(eng, shape, stride):
    """7 steps with batches 8, 8, 5, 8, 8, 5, 8 over 21 rows (ragged, two epoch changes), then 7 more from slot 7, with a
    (14, P) rate table whose entries are all different: theta, mean, sq_mean and every loss equal the step calls bit for
    bit."""
    dims, acts, loss, P = RUN_SHAPES[shape]
    spec = eng.MLPSpec(dims, acts, loss)
    D, B, N, seed, n0 = spec.n_params, 8, 21, 29, 3
    rng = np.random.default_rng(5)
    x = dev(rng.normal(size=(N, dims[0])))
    y = dev(rng.integers(0, dims[-1], size=N), torch.int32)
    sizes = ([8, 8, 5] * 5)[:14]                     # epochs of 21 rows; the second call goes on inside the third epoch
    rates = lc.run_rate_table(14, P)
    table = np.zeros((14, B), dtype=np.int32)
    s = 0
    while s < 14:                                    # an epoch = a permutation of the 21 rows in batches of 8, 8, 5
        perm, o = rng.permutation(N), 0
        for b in (8, 8, 5):
            if s < 14:
                assert sizes[s] == b
                table[s, :b] = perm[o:o + b]
                o, s = o + b, s + 1
    start = {"theta": (rng.normal(size=(P, D)) * 0.5).astype(np.float32), "mean": rng.normal(size=(P, D)).astype(np.float32),
             "sq": rng.uniform(1.0, 2.0, size=(P, D)).astype(np.float32)}
    plan = eng.MLPPlan(spec, max_batch=B, max_particles=P)
    table_dev = dev(table, torch.int32)

    def fresh():
        return {k: Guarded(v, True) for k, v in start.items()}

    st = fresh()
    step_losses = Guarded(np.zeros((14, P)), True)
    snap = {}
    for s in range(14):
        plan.sgld_lanes_step(st["theta"].t, st["mean"].t, st["sq"].t, x, y, rates[s], n0 + s, seed, step_losses.t[s],
                             seed_stride=stride, batch=sizes[s], row_idx=table_dev[s, :sizes[s]])
        if s in (6, 13):
            snap[s] = {k: v.get() for k, v in st.items()}
    assert all(g.intact() for g in list(st.values()) + [step_losses])
    step_losses = step_losses.get()
    assert np.all(np.isfinite(step_losses)) and len({step_losses[0, c].tobytes() for c in range(P)}) == P
    rt = fresh()
    losses = Guarded(np.full((14, P), SENTINEL), True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        plan.sgld_lanes_run(rt["theta"].t, rt["mean"].t, rt["sq"].t, x, y, table_dev, sizes[:7], rates[:7], n0, seed, losses.t,
                            seed_stride=stride)
        assert plan.last_run_path() == ("eager", 7)
    stream.synchronize()
    lo = losses.get()
    for k in rt:
        assert np.array_equal(bits(rt[k].get()), bits(snap[6][k])), f"{shape} stride {stride}: {k} after 7 steps"
    assert np.array_equal(bits(lo[:7]), bits(step_losses[:7])) and np.all(lo[7:] == SENTINEL)
    with torch.cuda.stream(stream):                 # ... and on from slot 7
        plan.sgld_lanes_run(rt["theta"].t, rt["mean"].t, rt["sq"].t, x, y, table_dev, sizes[7:], rates[7:], n0 + 7, seed,
                            losses.t, seed_stride=stride, slot0=7)
        assert plan.last_run_path() == ("eager", 7)
    stream.synchronize()
    for k in rt:
        assert np.array_equal(bits(rt[k].get()), bits(snap[13][k])), f"{shape} stride {stride}: {k} after 14 steps"
    assert np.array_equal(bits(losses.get()), bits(step_losses))
    assert all(g.intact() for g in list(rt.values()) + [losses])
    plan.check_finite()
    plan.close()


@pytest.mark.parametrize("name", ("f_d25_odd_p2", "f_d66_gathered_p5"))
def test_lanes_run_with_equal_rates_is_the_chains_run_bit_for_bit(eng, name):
    """Three steps with batches (full, full - 2, full) from the case's start, the device drawing the noise: sgld_lanes_run
    with seed_stride 1 and every lane of step s at the chains run's lrs[s] leaves theta, mean, sq_mean and the (3, P) loss
    rows of sgld_chains_run bit for bit, and both report three eager steps and no graph launch."""
    case = lc.CASE_BY_NAME[name]
    data = lc.chains_data(case)
    s0 = lc.initial_state(data)
    run = Run(eng, case, data)
    st, P = case.step, case.P
    sizes = [st.batch, st.batch - 2, st.batch]
    rows = data.step.idx if data.step.idx is not None else np.arange(st.batch)
    table = np.zeros((3, st.max_batch), dtype=np.int32)
    table[:, :st.batch] = rows[:st.batch]
    table_dev = dev(table, torch.int32)
    lrs = [float(np.float32(st.lr / (1.0 + 0.25 * s))) for s in range(3)]        # a rate per step, all different
    rates = np.repeat(np.asarray(lrs, dtype=np.float32)[:, None], P, axis=1)
    b, got = run.bufs, {}
    for which in ("chains", "lanes"):
        run.set_state(s0)
        losses = Guarded(np.full((3, P), SENTINEL), True)
        if which == "chains":
            run.plan.sgld_chains_run(b["theta"].t, b["mean"].t, b["sq"].t, run.x, run.y, table_dev, sizes, lrs, st.n0, st.seed,
                                     losses.t)
        else:
            run.plan.sgld_lanes_run(b["theta"].t, b["mean"].t, b["sq"].t, run.x, run.y, table_dev, sizes, rates, st.n0, st.seed,
                                    losses.t, seed_stride=1)
        assert run.plan.last_run_path() == ("eager", 3) and run.plan.last_run_graph_launches() == 0, which
        got[which] = run.get_state()
        got[which]["loss"] = losses.get()
        assert losses.intact() and run.guards_broken() == [], which
    assert np.all(np.isfinite(got["chains"]["loss"])) and not np.array_equal(bits(got["chains"]["theta"]), bits(s0["theta"]))
    for key in ("theta", "mean", "sq", "loss"):
        assert np.array_equal(bits(got["lanes"][key]), bits(got["chains"][key])), f"{name}: {key} differs from sgld_chains_run"
    run.plan.check_finite()
    run.plan.close()


def test_shape_errors(eng):
    from bayesian_inference_for_nn_amd._lib import PyzError, check, ptr
    import ctypes as C
    spec = eng.MLPSpec((3, 4, 2), ("tanh", "softmax"), "scce")
    plan = eng.MLPPlan(spec, max_batch=8, max_particles=2)
    D = spec.n_params
    th = torch.zeros((3, D), device="cuda")
    x, y, lo = torch.zeros((8, 3), device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(3, device="cuda")
    rates = (C.c_float * 3)(0.1, 0.1, 0.1)
    for batch, P in ((8, 3), (9, 2)):                 # more lanes than the plan's particles; a batch outside the plan
        rc = plan.lib.pyz_sgld_lanes_step(plan.h, ptr(th), ptr(th), ptr(th), P, ptr(x), ptr(y), None, batch, rates, 0, 1, 0, None,
                                          ptr(lo), None)
        assert rc == -2                               # PYZ_E_SHAPE
        with pytest.raises(PyzError):
            check(rc)
    idx = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    sizes = (C.c_int32 * 1)(8)
    rc = plan.lib.pyz_sgld_lanes_run(plan.h, ptr(th), ptr(th), ptr(th), 3, ptr(x), ptr(y), ptr(idx), sizes, rates, 1, 0, 0, 1, 0,
                                     ptr(lo), None)
    assert rc == -2
    assert torch.count_nonzero(th).item() == 0 and torch.count_nonzero(lo).item() == 0      # nothing ran
    # the engine refuses the same before the library sees it, and rates of the wrong shape
    th2, lo2 = torch.zeros((2, D), device="cuda"), torch.zeros(2, device="cuda")
    with pytest.raises(ValueError):
        plan.sgld_lanes_step(th, th, th, x, y, [0.1, 0.1, 0.1], 0, 1, lo)
    with pytest.raises(ValueError):
        plan.sgld_lanes_step(th2, th2, th2, x, y, [0.1, 0.1, 0.1], 0, 1, lo2)
    with pytest.raises(ValueError):
        plan.sgld_lanes_step(th2, th2, th2, x, y, [0.1, 0.1], 0, 1, lo2, seed_stride=2)
    plan.close()
