"""BBB lanes on the device: pyz_bbb_lanes_step against the float64 restatement (tests/bbb_lanes_checks.py lists the cases and
says which steps are taken), what a lane shares bit for bit with pyz_bbb_step, no cross-talk between lanes, the order of the
lanes, pyz_bbb_lanes_run against the step calls bit for bit, and the surface above them: BBB.compile(lanes=...), lane_scores,
lane_results and a grid search through BBBGridObjective on a 2 -> 16 -> 2 two-moons toy.

Every bound of a step is step_cases.compare_step's bound on one single BBB step.  Every buffer the kernels write sits between
sentinels, and the sentinels stay.

lane_scores("mu") against float64 NumPy: the loss within REL = 1e-4 relative and the error counts exact where no row is a
near-tie (GAP = 1e-4) -- the bound and the condition under which tests/test_gpu_lane_scores.py holds plan.lane_scores, which
is what SGLD.lane_scores and BBB.lane_scores both call."""

import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bbb_lanes_checks as bl  # noqa: E402
import bce_checks  # noqa: E402
from oracle import mlp as o_mlp  # noqa: E402

SENTINEL = -12345.0
TAIL = 64
REL, GAP = 1e-4, 1e-4


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
        self.bufs = {k: Guarded(zero, st.aligned) for k in ("mu", "rho", "w")}
        self.eps = Guarded(zero, st.aligned)
        self.cost = Guarded(np.zeros((self.P, 4)), True)
        self.pm_vec = dev(data.step.pm_vec) if st.prior_vec else None
        self.pr_vec = dev(data.step.pr_vec) if st.prior_vec else None

    def set_state(self, s):
        for k, b in self.bufs.items():
            b.set(s[k])

    def get_state(self):
        return {k: b.get() for k, b in self.bufs.items()}

    def guards_broken(self):
        return [k for k, b in list(self.bufs.items()) + [("eps", self.eps), ("cost", self.cost)] if not b.intact()]

    def step(self, k, eps, tables, stride):
        st, b = self.case.step, self.bufs
        z = None
        if eps is not None:
            self.eps.set(eps)
            z = self.eps.t
        self.cost.t.fill_(SENTINEL)
        self.plan.bbb_lanes_step(b["mu"].t, b["rho"].t, b["w"].t, self.x, self.y, tables.lr, tables.alpha, tables.prior_mean,
                                 tables.prior_rho, st.n0 + k, st.seed, self.cost.t, seed_stride=stride, batch=st.batch,
                                 row_idx=self.rid, eps=z, prior_mean_vec=self.pm_vec, prior_rho_vec=self.pr_vec)
        got = self.get_state()
        got["cost"] = self.cost.get()
        return got


def check_steps(run, case, data, stride, variant, walk, worst):
    """Steps n0 .. n0 + 2, each from the case's start (walk: one after the other, the reference restarting from the state
    read back), through compare_bbb_lanes_step."""
    tables = bl.lane_tables(case)
    run.set_state(bl.initial_state(data))
    for k in range(bl.N_STEPS):
        what = f"{case.name} stride {stride} {variant} step {k}{' of the walk' if walk else ''}"
        if not walk:
            run.set_state(bl.initial_state(data))
        s0 = run.get_state()
        got = run.step(k, bl.injected_noise(case, variant, k, stride), tables, stride)
        assert np.all(got["cost"][:, 3] == 0.0), f"{what}: the fourth cost column is {got['cost'][:, 3]}"
        ref = bl.ref_bbb_lanes_step(case, data, variant, k, s0, stride)
        rep = bl.compare_bbb_lanes_step(case, k, s0, got, ref, stride, what=f"stride {stride} {variant}: ")
        for q, r in sorted(rep.items()):
            print(f"{what}: {q}: error / tolerance {r:.4f}")
            worst[q] = max(worst.get(q, 0.0), r)
        assert run.guards_broken() == [], f"{what}: wrote outside {run.guards_broken()}"


@pytest.mark.parametrize("case", bl.CASES, ids=[c.name for c in bl.CASES])
def test_step_case(eng, case):
    data = bl.lanes_data(case)
    run = Run(eng, case, data)
    worst = {}
    for stride in bl.STRIDES:
        for variant in bl.VARIANTS:
            check_steps(run, case, data, stride, variant, False, worst)
            if case.name in bl.WALK:
                check_steps(run, case, data, stride, variant, True, worst)
    print(f"CASE | {case.name} | " + " | ".join(f"{q} {r:.4f}" for q, r in sorted(worst.items())))
    run.plan.check_finite()
    run.plan.close()


@pytest.mark.parametrize("case", bl.CASES, ids=[c.name for c in bl.CASES])
def test_a_lane_has_the_sampled_weights_and_the_kl_of_the_single_step_bit_for_bit(eng, case):
    """Lane c of a lanes step against pyz_bbb_step from row c of the state with lane c's numbers and seed: w and cost[2]
    (log q - log p) are the same bits, with the stream injected and with the device drawing it; and the same lanes step
    again gives the same bits throughout."""
    data = bl.lanes_data(case)
    s0 = bl.initial_state(data)
    run = Run(eng, case, data)
    st, P, D = case.step, case.P, case.D
    tables = bl.lane_tables(case)
    one = {k: torch.zeros(D, device="cuda") for k in ("mu", "rho", "w")}
    cost1 = torch.zeros(4, device="cuda")
    for stride in bl.STRIDES:
        for variant in bl.VARIANTS:
            eps = bl.injected_noise(case, variant, 1, stride)
            run.set_state(s0)
            got = run.step(1, eps, tables, stride)
            run.set_state(s0)
            again = run.step(1, eps, tables, stride)
            for key in ("mu", "rho", "w", "cost"):
                assert np.array_equal(bits(got[key]), bits(again[key])), f"{case.name} {variant}: repeating the step moves {key}"
            for c in range(P):
                for key in ("mu", "rho"):
                    one[key].copy_(dev(s0[key][c]))
                one["w"].zero_()
                run.plan.bbb_step(one["mu"], one["rho"], one["w"], run.x, run.y, float(tables.lr[c]), float(tables.alpha[c]),
                                  float(tables.prior_mean[c]), float(tables.prior_rho[c]), st.n0 + 1, st.seed + c * stride, cost1,
                                  batch=st.batch, row_idx=run.rid, eps=None if eps is None else dev(eps[c]),
                                  prior_mean_vec=run.pm_vec, prior_rho_vec=run.pr_vec)
                what = f"{case.name} stride {stride} {variant} lane {c}"
                assert np.array_equal(bits(one["w"].cpu().numpy()), bits(got["w"][c])), f"{what}: w differs from pyz_bbb_step"
                assert np.array_equal(bits(cost1.cpu().numpy()[2]), bits(got["cost"][c][2])), \
                    f"{what}: log q - log p {got['cost'][c][2]!r} against pyz_bbb_step's {cost1.cpu().numpy()[2]!r}"
    assert run.guards_broken() == []
    run.plan.close()


def test_a_workgroup_that_walks_several_blocks_keeps_the_bits_of_the_single_step(eng):
    """The grid gives a lane at most 8 * CUs / P workgroups, so with the library's 64 lanes a row of more than
    32 * 1024 elements (256 CUs) has workgroups that walk more than one block of 1024 -- the one path the small cases do not
    reach.  100 -> 330 -> 10 has D = 36 640, 36 blocks.  Lanes 0, 31 and 63 against pyz_bbb_step: w and log q - log p bit for
    bit, the device drawing eps, stride 1: a block skipped, walked twice or stored at another lane's place shows.  (How
    the float64 partials are grouped does not: their sums agree to far below the float32 rounding of the result.)"""
    from bayesian_inference_for_nn_amd import _lib
    spec = eng.MLPSpec((100, 330, 10), ("tanh", "softmax"), "scce")
    P, D, B, seed, step = _lib.MAX_LANES, spec.n_params, 8, 41, 6
    assert D == 36640 and -(-(-(-D // 4)) // 256) == 36
    rng = np.random.default_rng(12)
    x = dev(rng.normal(size=(B, 100)))
    y = dev(rng.integers(0, 10, size=B), torch.int32)
    mu0 = (rng.normal(size=(P, D)) * 0.1).astype(np.float32)
    rho0 = rng.uniform(-3.0, 0.0, size=(P, D)).astype(np.float32)
    tabs = [np.array([v * (1.0 + c / 64.0) for c in range(P)], dtype=np.float32) for v in (0.01, 0.0625, 0.125, 0.75)]
    plan = eng.MLPPlan(spec, max_batch=B, max_particles=P)
    mu, rho, w = Guarded(mu0, True), Guarded(rho0, True), Guarded(np.zeros((P, D)), True)
    cost = Guarded(np.zeros((P, 4)), True)
    plan.bbb_lanes_step(mu.t, rho.t, w.t, x, y, *tabs, step, seed, cost.t, seed_stride=1)
    got_w, got_cost = w.get(), cost.get()
    assert np.all(np.isfinite(got_cost)) and all(g.intact() for g in (mu, rho, w, cost))
    cost1, w1 = torch.zeros(4, device="cuda"), torch.zeros(D, device="cuda")
    for c in (0, 31, 63):
        plan.bbb_step(dev(mu0[c]), dev(rho0[c]), w1, x, y, float(tabs[0][c]), float(tabs[1][c]), float(tabs[2][c]),
                      float(tabs[3][c]), step, seed + c, cost1)
        assert np.array_equal(bits(w1.cpu().numpy()), bits(got_w[c])), f"lane {c}: w differs from pyz_bbb_step"
        assert np.array_equal(bits(cost1.cpu().numpy()[2]), bits(got_cost[c][2])), \
            f"lane {c}: log q - log p {got_cost[c][2]!r} against pyz_bbb_step's {cost1.cpu().numpy()[2]!r}"
    plan.close()


@pytest.mark.parametrize("name", ("f_d404_p5", "u_d1100_p5", "f_d25_odd_p2"))
def test_equal_lanes_on_one_stream_stay_equal(eng, name):
    """Stride 0: rows 0 and P - 1 start equal and carry equal hyper-parameters, the rows between others.  After three steps
    the two are equal bit for bit (one batch, one eps stream); with stride 1 they are not."""
    case = bl.CASE_BY_NAME[name]
    data = bl.lanes_data(case)
    s0 = bl.initial_state(data)
    last = case.P - 1
    for key in s0:
        s0[key][last] = s0[key][0]
    t = bl.lane_tables(case)
    t = bl.LaneTables(*(np.concatenate([a[:last], a[:1]]) for a in t))
    run = Run(eng, case, data)
    for stride in (0, 1):
        run.set_state(s0)
        for k in range(3):
            got = run.step(k, None, t, stride)
        equal = all(np.array_equal(bits(got[key][0]), bits(got[key][last])) for key in ("mu", "rho", "w", "cost"))
        assert equal == (stride == 0), f"{name} stride {stride}: rows 0 and {last} {'differ' if stride == 0 else 'are equal'}"
        if case.P > 2:
            assert not np.array_equal(bits(got["mu"][0]), bits(got["mu"][1]))
    assert run.guards_broken() == []
    run.plan.close()


@pytest.mark.parametrize("name", ("f_d66_gathered_p5", "u_d165_mse_p5", "f_d25_odd_p2"))
def test_reversed_lanes_give_the_reversed_rows(eng, name):
    """Lanes [a, b, c] against [c, b, a] -- state rows, tables and the injected eps reversed alike, stride 0: every row comes
    out with the same bits at its new place (a row's alignment moves with its place; its bits do not)."""
    case = bl.CASE_BY_NAME[name]
    data = bl.lanes_data(case)
    s0 = bl.initial_state(data)
    t = bl.lane_tables(case)
    run = Run(eng, case, data)
    eps = bl.injected_noise(case, "philox", 1, 0)
    eps = np.stack([np.roll(eps[c], c) for c in range(case.P)])           # stride 0 injects ONE stream: a row of its own each
    run.set_state(s0)
    got = run.step(1, eps, t, 0)
    run.set_state({k: v[::-1].copy() for k, v in s0.items()})
    rev = run.step(1, eps[::-1].copy(), bl.LaneTables(*(a[::-1].copy() for a in t)), 0)
    for key in ("mu", "rho", "w", "cost"):
        assert np.array_equal(bits(rev[key]), bits(got[key][::-1])), f"{name}: {key} depends on the order of the lanes"
    assert len({got["mu"][c].tobytes() for c in range(case.P)}) == case.P
    assert run.guards_broken() == []
    run.plan.close()


# ---------------------------------------------------------------- the run
RUN_SHAPES = {
    "fused_p3": ((5, 7, 3), ("tanh", "softmax"), "scce", 3),
    "unfused_p2": ((3, 5, 33), ("tanh", "softmax"), "scce", 2),
}


@pytest.mark.parametrize("shape", sorted(RUN_SHAPES))
@pytest.mark.parametrize("stride", bl.STRIDES)
def test_run_equals_step_calls_bit_for_bit(eng, shape, stride):
    """7 steps with batches 9, 9, 5, 9, 9, 5, 9 over 23 rows (ragged, two epoch changes) from slot 3 of a (12, P, 4) cost
    buffer: mu, rho, w and every cost equal the 7 step calls bit for bit, the costs land in slots 3 .. 9 and no other."""
    dims, acts, loss, P = RUN_SHAPES[shape]
    spec = eng.MLPSpec(dims, acts, loss)
    D, B, N, seed, step0, slot0, slots = spec.n_params, 9, 23, 29, 3, 3, 12
    rng = np.random.default_rng(5)
    x = dev(rng.normal(size=(N, dims[0])))
    y = dev(rng.integers(0, dims[-1], size=N), torch.int32)
    sizes = list(bl.RUN_SIZES)
    n_steps = len(sizes)
    table = np.zeros((slots, B), dtype=np.int32)
    s = 0
    while s < n_steps:                               # an epoch = a permutation of the 23 rows in batches of 9, 9, 5
        perm, o = rng.permutation(N), 0
        for b in (9, 9, 5):
            if s < n_steps:
                assert sizes[s] == b
                table[slot0 + s, :b] = perm[o:o + b]
                o, s = o + b, s + 1
    tabs = bl.LaneTables(*(np.array(v[:P], dtype=np.float32) for v in ((0.05, 0.03, 0.02), (0.0625, 0.125, 0.03125),
                                                                         (0.0, 0.125, -0.25), (0.5, 0.25, -0.5))))
    start = {"mu": (rng.normal(size=(P, D)) * 0.5).astype(np.float32), "rho": rng.uniform(-3.0, 0.0, size=(P, D)).astype(np.float32),
             "w": np.zeros((P, D), dtype=np.float32)}
    plan = eng.MLPPlan(spec, max_batch=B, max_particles=P)
    table_dev = dev(table, torch.int32)

    def fresh():
        return {k: Guarded(v, True) for k, v in start.items()}

    st = fresh()
    step_costs = Guarded(np.zeros((n_steps, P, 4)), True)
    for s in range(n_steps):
        plan.bbb_lanes_step(st["mu"].t, st["rho"].t, st["w"].t, x, y, *tabs, step0 + s, seed, step_costs.t[s], seed_stride=stride,
                            batch=sizes[s], row_idx=table_dev[slot0 + s, :sizes[s]])
    assert all(g.intact() for g in list(st.values()) + [step_costs])
    want = {k: v.get() for k, v in st.items()}
    step_costs = step_costs.get()
    assert np.all(np.isfinite(step_costs)) and len({step_costs[0, c].tobytes() for c in range(P)}) == P
    rt = fresh()
    costs = Guarded(np.full((slots, P, 4), SENTINEL), True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        plan.bbb_lanes_run(rt["mu"].t, rt["rho"].t, rt["w"].t, x, y, table_dev, sizes, *tabs, step0, seed, costs.t,
                           seed_stride=stride, slot0=slot0)
        assert plan.last_run_path() == ("eager", n_steps) and plan.last_run_graph_launches() == 0
    stream.synchronize()
    for k in rt:
        assert np.array_equal(bits(rt[k].get()), bits(want[k])), f"{shape} stride {stride}: {k} after {n_steps} steps"
    co = costs.get()
    assert np.array_equal(bits(co[slot0:slot0 + n_steps]), bits(step_costs))
    assert np.all(co[:slot0] == SENTINEL) and np.all(co[slot0 + n_steps:] == SENTINEL)
    assert all(g.intact() for g in list(rt.values()) + [costs])
    plan.check_finite()
    plan.close()


def test_shape_errors(eng):
    from bayesian_inference_for_nn_amd._lib import MAX_LANES, PyzError, check, ptr
    import ctypes as C
    spec = eng.MLPSpec((3, 4, 2), ("tanh", "softmax"), "scce")
    plan = eng.MLPPlan(spec, max_batch=8, max_particles=2)
    D = spec.n_params
    big = MAX_LANES + 1
    th = torch.zeros((big, D), device="cuda")
    x, y = torch.zeros((8, 3), device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    co = torch.zeros((big, 4), device="cuda")
    tab = (C.c_float * big)(*([0.1] * big))
    idx = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    sizes = (C.c_int32 * 1)(8)
    for P in (3, big):                                # more lanes than the plan's particles; more than the library takes
        rc = plan.lib.pyz_bbb_lanes_step(plan.h, ptr(th), ptr(th), ptr(th), P, ptr(x), ptr(y), None, 8, tab, tab, tab, tab, None, None,
                                         0, 1, 0, None, ptr(co), None)
        assert rc == -2                               # PYZ_E_SHAPE
        with pytest.raises(PyzError):
            check(rc)
        rc = plan.lib.pyz_bbb_lanes_run(plan.h, ptr(th), ptr(th), ptr(th), P, ptr(x), ptr(y), tab, tab, tab, tab, None, None,
                                        ptr(idx), sizes, 1, 0, 0, 1, 0, ptr(co), None)
        assert rc == -2
    rc = plan.lib.pyz_bbb_lanes_step(plan.h, ptr(th), ptr(th), ptr(th), 2, ptr(x), ptr(y), None, 9, tab, tab, tab, tab, None, None,
                                     0, 1, 0, None, ptr(co), None)
    assert rc == -2                                   # a batch outside the plan
    assert torch.count_nonzero(th).item() == 0 and torch.count_nonzero(co).item() == 0      # nothing ran
    th2, co2 = torch.zeros((2, D), device="cuda"), torch.zeros((2, 4), device="cuda")
    with pytest.raises(ValueError):
        plan.bbb_lanes_step(th, th, th, x, y, [0.1] * big, [0.1] * big, [0.0] * big, [0.0] * big, 0, 1, co)
    with pytest.raises(ValueError):
        plan.bbb_lanes_step(th2, th2, th2, x, y, [0.1] * 3, [0.1] * 2, [0.0] * 2, [0.0] * 2, 0, 1, co2)
    with pytest.raises(ValueError):
        plan.bbb_lanes_step(th2, th2, th2, x, y, [0.1] * 2, [0.1] * 2, [0.0] * 2, [0.0] * 2, 0, 1, co2, seed_stride=2)
    with pytest.raises(ValueError):
        plan.bbb_lanes_step(th2, th2, th2, x, y, [0.1] * 2, [0.1] * 2, [0.0] * 2, [0.0] * 2, 0, 1, co2, prior_mean_vec=th2[0])
    plan.close()


# ---------------------------------------------------------------- the optimizer's surface, on two moons
BASE = dict(lr=0.05, alpha=0.01, batch_size=48)
LANES = [{"lr": 0.1}, {"alpha": 0.002, "pi": 0.5}, {"lr": 0.02, "alpha": 0.05}]
NEW = ("bbb_lanes_step", "bbb_lanes_run")
OLD = ("bbb_step", "bbb_run")


def moons():
    from bayesian_inference_for_nn_amd import synth
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
    from bayesian_inference_for_nn_amd.nn import sequential_json
    x, y = synth.moons(200, seed=42)
    return Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=3), sequential_json(2, [16, 2], ["relu", "softmax"])


def compiled(seed=17, base=BASE, **kw):
    from bayesian_inference_for_nn_amd.distributions import GaussianPrior
    from bayesian_inference_for_nn_amd.optimizers import BBB
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    ds, cfg = moons()
    opt = BBB()
    opt.compile(HyperParameters(**base), cfg, ds, verbose=False, seed=seed, prior=GaussianPrior(0.0, -3.0),
                prior2=GaussianPrior(0.0, -1.0), **kw)
    return opt


def count_calls(opt, names=NEW + OLD):
    calls = {name: 0 for name in names}
    for name in calls:
        inner = getattr(opt._plan, name)

        def wrapper(*a, _inner=inner, _name=name, **kw):
            calls[_name] += 1
            return _inner(*a, **kw)
        setattr(opt._plan, name, wrapper)
    return calls


def test_quiet_train_equals_step_calls_bit_for_bit(gpu_device):
    from bayesian_inference_for_nn_amd.optimizers.BBB import mix_prior
    P, n = len(LANES), 12
    a, b = compiled(lanes=LANES), compiled(lanes=LANES)
    assert a._mu.shape == (P, a._D) and a._plan.max_particles == P
    # every lane starts from its own mixed prior
    mixed = mix_prior(a._prior, a._prior2, 0.5)
    assert mixed._std_dev != a._prior._std_dev
    rho0 = a._rho.cpu().numpy()
    assert np.all(rho0[0] == np.float32(-3.0)) and np.all(rho0[1] == np.float32(mixed._std_dev)) and np.all(rho0[2] == rho0[0])
    assert float(a._lane_tabs[3][1]) == float(np.float32(mixed._std_dev)) and a._lane_tabs[0].tolist() == [np.float32(0.1), np.float32(0.05), np.float32(0.02)]
    calls_a, calls_b = count_calls(a), count_calls(b)
    a.train(n)                                        # quiet: pyz_bbb_lanes_run through _run_resident_chunks
    for _ in range(n):
        ret = b.step()
    assert calls_a == {"bbb_step": 0, "bbb_run": 0, "bbb_lanes_step": 0, "bbb_lanes_run": 1}
    assert calls_b == {"bbb_step": 0, "bbb_run": 0, "bbb_lanes_step": n, "bbb_lanes_run": 0}
    for name in ("_mu", "_rho", "_w", "_cost"):
        assert np.array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy())), name
    ca, cb = a.lane_costs().cpu().numpy(), b.lane_costs().cpu().numpy()
    assert ca.shape == (n, P, 4) and np.array_equal(bits(ca), bits(cb)) and np.all(np.isfinite(ca))
    assert float(ret) == float(cb[-1, 0, 0])                              # step() returns lane 0's cost
    assert a._step == b._step == n and a.train_losses == [] and a.val_losses == []
    mu = a._mu.cpu().numpy()
    assert len({mu[c].tobytes() for c in range(P)}) == P                  # the lanes did take their own numbers
    with pytest.raises(ValueError):
        a.result()
    results = a.lane_results()
    assert len(results) == P
    for c, res in enumerate(results):
        model, tl, vl = res
        d = model._distributions[0]._tf_distribution
        sl = a._spec.layer_slices()[0]
        assert np.array_equal(d.loc, mu[c][sl]) and tl == [] and vl == []
    # a second quiet train goes on from the first (slots and Philox steps), as more step calls do
    a.train(5)
    for _ in range(5):
        b.step()
    assert np.array_equal(bits(a._mu.cpu().numpy()), bits(b._mu.cpu().numpy())) and a.lane_costs().shape == (n + 5, P, 4)
    assert np.array_equal(bits(a.lane_costs().cpu().numpy()), bits(b.lane_costs().cpu().numpy()))


def test_lane_scores_mu_against_numpy_and_predictive_against_the_lane_models(gpu_device):
    from bayesian_inference_for_nn_amd.distributions import tfd
    P = len(LANES)
    opt = compiled(lanes=LANES)
    opt.train(30)
    spec = o_mlp.MLPSpec(opt._spec.dims, opt._spec.acts, "scce")
    mu = opt._mu.cpu().numpy().astype(np.float64)
    for split in ("valid", "train"):
        x, y = (getattr(opt._dataset, split + "_data") if split != "train" else opt._dataset.training_dataset()).as_numpy()
        x, y = np.asarray(x, dtype=np.float32).reshape(len(x), -1), np.asarray(y).reshape(-1).astype(np.int32)
        got = opt.lane_scores(split=split, weights="mu")
        assert got["n"] == len(x) and got["loss"].shape == (P,) and got["loss"].dtype == np.float64
        for c in range(P):
            loss, _, out = o_mlp.loss_and_grad(mu[c], x.astype(np.float64), y, spec, np.float64)
            top = np.sort(out, axis=1)
            assert (top[:, -1] - top[:, -2]).min() >= GAP, "a row is a near-tie: the error count is not defined to a row"
            rel = abs(got["loss"][c] - loss) / abs(loss)
            print(f"SCORES | {split} lane {c} | loss error / bound {rel / REL:.4f}")
            assert rel <= REL, (split, c, got["loss"][c], loss)
            assert got["error"][c] == float((np.argmax(out, axis=1) != y).sum()) / len(x)
    assert len(x) > opt._plan.max_batch                                   # the train split took more than one chunk
    # predictive: the draws and the read-out of lane_results()[c].predict from the same seed
    xv, yv = opt._dataset.valid_data.as_numpy()
    xv, yv = np.asarray(xv, dtype=np.float32).reshape(len(xv), -1), np.asarray(yv).reshape(-1)
    tfd.seed(5)
    got = opt.lane_scores(split="valid", weights="predictive", nb_samples=8)
    assert got["loss"] is None and got["n"] == len(xv)
    tfd.seed(5)
    for c, res in enumerate(opt.lane_results()):
        _, mean = res.predict(xv, nb_samples=8)
        wrong = int((np.argmax(np.asarray(mean), axis=1) != yv).sum())
        assert got["error"][c] == wrong / len(xv), (c, got["error"][c] * len(xv), wrong)
    for bad in ({"split": "all"}, {"weights": "theta"}, {"weights": "predictive", "nb_samples": 0}):
        with pytest.raises(ValueError):
            opt.lane_scores(**bad)


def test_distinct_seeds_are_the_single_optimizers_and_the_untouched_paths(gpu_device):
    """lane_seeds="distinct": lane c at the base point is the one-posterior BBB with seed + c in its eps stream (sampled
    weights and log q - log p bit for bit at the first step, from the same start and batch); without lanes nothing reaches
    the new methods."""
    a = compiled(lanes=[{}, {}], lane_seeds="distinct")
    assert a._lane_stride == 1 and compiled(lanes=[{}])._lane_stride == 0
    a.step()
    w, cost = a._w.cpu().numpy(), a._cost.cpu().numpy()
    assert not np.array_equal(w[0], w[1])
    plain = compiled()
    calls = count_calls(plain)
    plain.step()
    assert np.array_equal(bits(plain._w.cpu().numpy()), bits(w[0])) and np.array_equal(bits(plain._cost.cpu().numpy()[2]), bits(cost[0][2]))
    plain.train(6)
    assert calls["bbb_lanes_step"] == calls["bbb_lanes_run"] == 0 and calls["bbb_step"] + calls["bbb_run"] == 2
    plain.result()
    with pytest.raises(ValueError):
        plain.lane_scores()
    with pytest.raises(ValueError):
        plain.lane_results()


def test_grid_search_through_the_lanes(gpu_device):
    from bayesian_inference_for_nn_amd.distributions import GaussianPrior
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import BBBGridObjective, GridOptimizer, HyperParameters, Real
    ds, cfg = moons()
    hp = HyperParameters(**BASE)
    n, seed = 15, 23
    prior, prior2 = GaussianPrior(0.0, -3.0), GaussianPrior(0.0, -1.0)
    obj = BBBGridObjective(hp, cfg, ds, n, prior, prior2, metric="val_loss", weights="mu", seed=seed, max_lanes=4)
    grid = GridOptimizer()
    grid.compile(obj, Real(0.02, 0.1, "lr"), Real(0.0, 1.0, "alpha"), n=3, specify={"alpha": [0.002, 0.05]}, verbose=False)
    grid.optimize()
    eps = (0.1 - 0.02) / 2
    points = list(itertools.product([i * eps + 0.02 for i in range(3)], [0.002, 0.05]))
    assert obj.trainings == [4, 2]
    assert list(grid._results) == points
    assert all(isinstance(v, float) and np.isfinite(v) for v in grid._results.values())
    assert len(set(grid._results.values())) == len(points)
    for chunk in (points[:4], points[4:]):
        opt = compiled(seed=seed, lanes=[{"lr": lr, "alpha": al} for lr, al in chunk])
        opt.train(n)
        direct = opt.lane_scores(split="valid", weights="mu")["loss"]
        for p, v in zip(chunk, direct):
            assert grid._results[p] == float(v), p                        # bit for bit: the same float64
    point, value = grid.best()
    assert value == min(grid._results.values()) and grid._results[point] == value
    single = obj(0.05, names=["lr"])
    assert obj.trainings == [4, 2, 1] and np.isfinite(single)
    err = BBBGridObjective(hp, cfg, ds, 5, prior, prior2, metric="val_error", weights="predictive", nb_samples=4, seed=seed, max_lanes=4)
    out = err.evaluate_lanes(["lr", "pi", "batch_size"], [(0.02, 1.0, 48), (0.03, 0.5, 24), (0.04, 0.25, 48)])
    assert err.trainings == [2, 1] and all(0.0 <= v <= 1.0 for v in out)
