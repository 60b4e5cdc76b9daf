"""SGD / SWAG with P members per launch on the device: pyz_sgd_members_step and pyz_swag_members_step against the float64
restatement (tests/members_checks.py lists the cases), no cross-talk between the rows, the runs against the step calls bit
for bit, the argument errors, the optimizers' n_members surface and the Mixture read-out.

A step test is one case in one mode: three consecutive steps from n0 = 3 (SWAG: update into row 1, no update, update with
no row; SGD rows: hit, miss, hit).  Before every step the state is read back and the reference restarts from it, so every
bound is step_cases.compare_step's bound on one step of one model."""

import random
from math import sqrt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bce_checks  # noqa: E402
import members_checks as mc  # noqa: E402
import step_cases as sc  # noqa: E402
from head_cases import close_blocks  # noqa: E402

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
    """A float32 array of any shape as a view into a sentinel-filled buffer: one element in front (the array then starts
    4 bytes off 16-byte alignment) or four (aligned), 64 behind."""

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
    """The device side of one case in one mode: a plan for the case's P particles, the data and guarded state buffers
    for P (or fewer) members, the (P, K_DEV, D) deviations and the loss among them."""

    def __init__(self, eng, case, mode, data, P=None):
        self.case, self.mode, st = case, mode, case.step
        self.P = case.P if P is None else P
        spec = st.spec
        self.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=st.max_batch, max_particles=case.P)
        self.x = dev(data.step.x)
        self.y = dev(data.step.y, torch.int32 if spec.loss == "scce" else torch.float32)
        self.rid = dev(data.step.idx, torch.int32) if data.step.idx is not None else None
        zero = np.zeros((self.P, case.D))
        self.bufs = {k: Guarded(zero, st.aligned) for k in (("theta", "mean", "sq") if mode == "swag" else ("theta", "mean"))}
        if mode == "swag":
            self.bufs["dev"] = Guarded(np.zeros((self.P, mc.K_DEV, case.D)), st.aligned)
        self.loss = Guarded(np.zeros(self.P), True)

    def set_state(self, s):
        for k, b in self.bufs.items():
            b.set(s[k])

    def get_state(self):
        return {k: b.get() for k, b in self.bufs.items()}

    def guards_broken(self):
        return [k for k, b in list(self.bufs.items()) + [("loss", self.loss)] if not b.intact()]

    def step(self, k):
        st, b = self.case.step, self.bufs
        hit, col = mc.step_flags(self.mode, k)
        self.loss.t.zero_()
        if self.mode == "swag":
            self.plan.swag_members_step(b["theta"].t, b["mean"].t, b["sq"].t, b["dev"].t, self.x, self.y, st.lr, st.n0 + k, hit,
                                        col, self.loss.t, batch=st.batch, row_idx=self.rid)
        else:
            self.plan.sgd_members_step(b["theta"].t, b["mean"].t, self.x, self.y, st.lr, st.n0 + k, hit, self.loss.t,
                                       batch=st.batch, row_idx=self.rid)
        got = self.get_state()
        got["loss"] = self.loss.get()
        return got

    def close(self):
        self.plan.close()


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("case", mc.CASES, ids=[c.name for c in mc.CASES])
def test_step_case(eng, case, mode):
    data = mc.members_data(case)
    run = Run(eng, case, mode, data)
    run.set_state(mc.initial_state(case, mode, data))
    worst = {}
    for k in range(mc.N_STEPS):
        what = f"{case.name} {mode} step {k}"
        hit, col = mc.step_flags(mode, k)
        s0 = run.get_state()
        got = run.step(k)
        ref = mc.ref_members_step(case, data, mode, k, s0)
        rep = mc.compare_members_step(case, mode, k, s0, got, ref)
        for q, r in sorted(rep.items()):
            print(f"{what}: {q}: error / tolerance {r:.4f}")
            worst[q] = max(worst.get(q, 0.0), r)
        assert run.guards_broken() == [], f"{what}: wrote outside {run.guards_broken()}"
        # what a step must leave alone, over the whole buffers
        if not hit:
            for key in set(s0) - {"theta"}:
                assert np.array_equal(bits(got[key]), bits(s0[key])), f"{what}: {key} moved on a step that is no hit"
        elif mode == "swag":
            for c in range(case.P):
                for r in range(mc.K_DEV):
                    if r != col:
                        assert np.array_equal(bits(got["dev"][c, r]), bits(s0["dev"][c, r])), \
                            f"{what}: deviation row {r} of member {c}, which this step does not write"
        # the same step from the same state: the same bits
        run.set_state(s0)
        assert same_bits(got, run.step(k)), f"{what}: repeating the step from the same state gives other bits"
        assert run.guards_broken() == [], f"{what}: wrote outside {run.guards_broken()}"
    print(f"CASE | {case.name} | {mode} | " + " | ".join(f"{q} {r:.4f}" for q, r in sorted(worst.items())))
    run.close()


CROSS_TALK = ("f_d66_gathered_p5", "u_d165_mse_p5")


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("name", CROSS_TALK)
def test_no_cross_talk_between_members(eng, name, mode):
    """Row c of a P = 5 step depends on row c of the state alone.
    (a) With every OTHER row of every state buffer replaced, row c comes out with the same bits (same launch geometry).
    (b) Against a P = 1 call of the same entry point from the same start: the update is the same arithmetic, the gradient
        pass picks its kernels from the particle count as well, so the rows agree within compare_step; whether they also
        agree bit for bit at these shapes is printed, not asserted."""
    case = mc.CASE_BY_NAME[name]
    data = mc.members_data(case)
    s0 = mc.initial_state(case, mode, data)
    run = Run(eng, case, mode, data)
    one = Run(eng, case, mode, data, P=1)
    for k in (0, 1):
        run.set_state(s0)
        got = run.step(k)
        ref = mc.ref_members_step(case, data, mode, k, s0)
        for c in range(case.P):
            # (a)
            other = {key: np.roll(v, 1, axis=0) * np.float32(1.25) for key, v in s0.items()}
            for key in other:
                other[key][c] = s0[key][c]
            run.set_state(other)
            again = run.step(k)
            for key in got:
                assert np.array_equal(bits(again[key][c]), bits(got[key][c])), \
                    f"{name} {mode} step {k}: row {c} of {key} moved with the other rows"
            # (b)
            one.set_state({key: v[c:c + 1] for key, v in s0.items()})
            g1 = {key: v[0] for key, v in one.step(k).items()}
            s0_c, ref_c = mc.member_state(s0, c), mc.member_state(ref, c)
            sc.compare_step(case.step, mode, k, s0_c, g1, ref_c, what=f"P = 1 call, member {c}: ")
            sc.compare_step(case.step, mode, k, s0_c, mc.member_state(got, c),
                            {key: np.asarray(v, dtype=np.float64) for key, v in g1.items()}, what=f"row {c} of P = 5 against P = 1: ")
            eq = all(np.array_equal(bits(g1[key]), bits(got[key][c])) for key in g1)
            print(f"BITS | {name} | {mode} | step {k} | member {c} | P = 5 row against the P = 1 call: {'equal' if eq else 'different'}")
    assert run.guards_broken() == [] and one.guards_broken() == []
    run.close()
    one.close()


# ---------------------------------------------------------------- the runs
RUN_SHAPES = {
    "fused_p3": ((5, 7, 3), ("tanh", "softmax"), "scce", 3),
    "unfused_p2": ((3, 5, 33), ("tanh", "softmax"), "scce", 2),
}


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("shape", sorted(RUN_SHAPES))
def test_run_equals_step_calls_bit_for_bit(eng, shape, mode):
    """7 steps with batches 8, 8, 5, 8, 8, 5, 8 over 21 rows (ragged, two epoch changes), then 7 more from slot 7, from
    count 0 with frequency 3 and k = 3: the hits are the counts 0, 3, 6, 9, 12, so the three columns fill and the last is
    replaced twice.  theta, mean, sq_mean, all deviations and every loss row equal the step calls bit for bit, with
    use_graph 0 and 1; untouched loss slots keep the sentinel.  SGD rows: mean equals the weights after the last hit."""
    dims, acts, loss, P = RUN_SHAPES[shape]
    spec = eng.MLPSpec(dims, acts, loss)
    D, B, N, freq, K = spec.n_params, 8, 21, 3, 3
    swag = mode == "swag"
    rng = np.random.default_rng(5)
    x = dev(rng.normal(size=(N, dims[0])))
    y = dev(rng.integers(0, dims[-1], size=N), torch.int32)
    sizes = ([8, 8, 5] * 5)[:14]                     # epochs of 21 rows; the second call goes on inside the third epoch
    assert tuple(sizes[:7]) == mc.RUN_SIZES
    lrs = mc.run_lrs(14)
    assert len(set(lrs)) == 14
    table = np.zeros((14, B), dtype=np.int32)
    s = 0
    while s < 14:                                    # an epoch = a permutation of the 21 rows in batches of 8, 8, 5
        perm, o = rng.permutation(N), 0
        for b in (8, 8, 5):
            if s < 14:
                table[s, :b] = perm[o:o + b]
                o, s = o + b, s + 1
    table_dev = dev(table, torch.int32)
    start = {"theta": (rng.normal(size=(P, D)) * 0.5).astype(np.float32), "mean": rng.normal(size=(P, D)).astype(np.float32)}
    if swag:
        start["sq"] = rng.uniform(1.0, 2.0, size=(P, D)).astype(np.float32)
        start["dev"] = rng.normal(size=(P, K, D)).astype(np.float32)
    plan = eng.MLPPlan(spec, max_batch=B, max_particles=P)

    def fresh():
        return {k: dev(v) for k, v in start.items()}

    def run(t, lo, hi, losses, use_graph):
        if swag:
            plan.swag_members_run(t["theta"], t["mean"], t["sq"], t["dev"], freq, x, y, table_dev, sizes[lo:hi], lrs[lo:hi], lo,
                                  losses, use_graph=use_graph, slot0=lo)
        else:
            plan.sgd_members_run(t["theta"], t["mean"], freq, x, y, table_dev, sizes[lo:hi], lrs[lo:hi], lo, losses,
                                 use_graph=use_graph, slot0=lo)

    st = fresh()
    step_losses = torch.zeros((14, P), device="cuda")
    snap, n_cols, cols, after_hit = {}, 0, [], None
    for s in range(14):                              # the host's bookkeeping, as the optimizers' step() keeps it
        hit = s % freq == 0
        if swag:
            col = min(n_cols, K - 1)
            plan.swag_members_step(st["theta"], st["mean"], st["sq"], st["dev"], x, y, lrs[s], s, hit, col if hit else None,
                                   step_losses[s], batch=sizes[s], row_idx=table_dev[s, :sizes[s]])
            if hit:
                cols.append(col)
                n_cols = min(n_cols + 1, K)
        else:
            plan.sgd_members_step(st["theta"], st["mean"], x, y, lrs[s], s, hit, step_losses[s], batch=sizes[s],
                                  row_idx=table_dev[s, :sizes[s]])
        if hit:
            after_hit = st["theta"].cpu().numpy().copy()
        if s in (6, 13):
            snap[s] = {k: v.cpu().numpy().copy() for k, v in st.items()}
            if not swag:
                assert np.array_equal(bits(snap[s]["mean"]), bits(after_hit)), f"{shape}: SGD mean is not the weights after the last hit"
    assert not swag or cols == [0, 1, 2, 2, 2]
    step_losses = step_losses.cpu().numpy()
    assert np.all(np.isfinite(step_losses)) and len({step_losses[0, c].tobytes() for c in range(P)}) == P
    for use_graph in (False, True):
        rt = fresh()
        losses = torch.full((14, P), SENTINEL, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            run(rt, 0, 7, losses, use_graph)
            kind, steps = plan.last_run_path()
            assert steps == 7 and kind == "eager"
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in rt.items()}
        lo = losses.cpu().numpy()
        for k in got:
            assert np.array_equal(bits(got[k]), bits(snap[6][k])), f"{shape} {mode} use_graph={use_graph}: {k} after 7 steps"
        assert np.array_equal(bits(lo[:7]), bits(step_losses[:7])) and np.all(lo[7:] == SENTINEL)
        with torch.cuda.stream(stream):             # ... and on from slot 7
            run(rt, 7, 14, losses, use_graph)
            assert plan.last_run_path()[1] == 7
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in rt.items()}
        for k in got:
            assert np.array_equal(bits(got[k]), bits(snap[13][k])), f"{shape} {mode} use_graph={use_graph}: {k} after 14 steps"
        assert np.array_equal(bits(losses.cpu().numpy()), bits(step_losses))
    plan.check_finite()
    plan.close()


def test_shape_errors(eng):
    from bayesian_inference_for_nn_amd._lib import PyzError, check, ptr
    import ctypes as C
    spec = eng.MLPSpec((3, 4, 2), ("tanh", "softmax"), "scce")
    plan = eng.MLPPlan(spec, max_batch=8, max_particles=2)
    D, lib, h = spec.n_params, plan.lib, plan.h
    th = torch.zeros((3, D), device="cuda")
    dv = torch.zeros((3, 2, D), device="cuda")
    x, y, lo = torch.zeros((8, 3), device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros((2, 3), device="cuda")
    idx = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    bs, lr = (C.c_int32 * 1)(8), (C.c_float * 1)(0.1)

    def sgd_step(P=2, batch=8):
        return lib.pyz_sgd_members_step(h, ptr(th), ptr(th), P, ptr(x), ptr(y), None, batch, 0.1, 0, 1, ptr(lo), None)

    def swag_step(P=2, batch=8, k=2, d=dv):
        return lib.pyz_swag_members_step(h, ptr(th), ptr(th), ptr(th), ptr(d), k, P, ptr(x), ptr(y), None, batch, 0.1, 0, 1, 0,
                                         ptr(lo), None)

    def sgd_run(P=2, freq=1, sizes=bs):
        return lib.pyz_sgd_members_run(h, ptr(th), ptr(th), P, freq, ptr(x), ptr(y), ptr(idx), sizes, lr, 1, 0, 0, ptr(lo), 0, None)

    def swag_run(P=2, freq=1, k=2, d=dv, sizes=bs):
        return lib.pyz_swag_members_run(h, ptr(th), ptr(th), ptr(th), ptr(d), k, freq, P, ptr(x), ptr(y), ptr(idx), sizes, lr, 1,
                                        0, 0, ptr(lo), 0, None)

    nine = (C.c_int32 * 1)(9)
    for rc in (sgd_step(P=3), sgd_step(batch=9), swag_step(P=3), swag_step(batch=9), sgd_run(P=3), sgd_run(sizes=nine),
               swag_run(P=3), swag_run(sizes=nine)):
        assert rc == -2                               # PYZ_E_SHAPE: more members than the plan's particles; a batch outside it
        with pytest.raises(PyzError):
            check(rc)
    for rc in (swag_step(k=0), swag_run(k=0), sgd_run(freq=0), swag_run(freq=0), swag_step(d=None), swag_run(d=None)):
        assert rc == -1                               # PYZ_E_INVALID
    torch.cuda.synchronize()
    assert float(th.abs().max()) == 0.0 and float(dv.abs().max()) == 0.0      # no refused call touched the state
    plan.close()


# ---------------------------------------------------------------- the optimizers' surface
def regression():
    from bayesian_inference_for_nn_amd import synth
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import MeanSquaredError
    from bayesian_inference_for_nn_amd.nn import sequential_json
    x, y = synth.linreg(70)
    x, y = x / 20.0, y / 40.0
    return Dataset((x, y), MeanSquaredError, "Regression", seed=0), sequential_json(1, [5, 1], ["tanh", "linear"])


HP = {"SGD": dict(lr=0.02, frequency=3, batch_size=16), "SWAG": dict(lr=0.02, frequency=3, k=3, scale=0.5, batch_size=16)}
STATE = {"SGD": ("_theta", "_mean_dev"), "SWAG": ("_theta", "_mean_dev", "_sq_mean_dev", "_dev_rows")}
ENTRY = {"SGD": ("sgd_members_step", "sgd_members_run"), "SWAG": ("swag_members_step", "swag_members_run")}


def starting_model(cfg, seed=99):
    from bayesian_inference_for_nn_amd.nn.model import model_from_json
    net = model_from_json(cfg)
    net.reset_glorot(np.random.default_rng(seed))
    return net


def compiled(which, n_members, seed=17, start=None):
    from bayesian_inference_for_nn_amd import optimizers
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    ds, cfg = regression()
    opt = getattr(optimizers, which)()
    extra = {} if n_members is None else {"n_members": n_members}
    opt.compile(HyperParameters(**HP[which]), cfg, ds, verbose=False, seed=seed,
                starting_model=starting_model(cfg) if start is None else start, **extra)
    return opt


def count_calls(opt, which):
    """Counting wrappers on the plan's two new methods of this optimizer."""
    calls = {name: 0 for name in ENTRY[which]}
    for name in calls:
        inner = getattr(opt._plan, name)

        def wrapper(*a, _inner=inner, _name=name, **kw):
            calls[_name] += 1
            return _inner(*a, **kw)
        setattr(opt._plan, name, wrapper)
    return calls


def state_of(opt, which):
    return {name: getattr(opt, name).cpu().numpy().copy() for name in STATE[which]}


def lowrank_params(opt, mean, sq, dev, sl=slice(None)):
    """What SWAG.result() gives MultivariateNormalDiagPlusLowRank from one member's rows, restricted to a slice."""
    return (mean[sl], sq[sl] - mean[sl] ** 2,
            np.asarray(sqrt(opt._scale / (opt._k - 1)) * dev[:opt._n_cols][:, sl].T, dtype=np.float32))


@pytest.mark.parametrize("which", ["SGD", "SWAG"])
def test_surface_with_three_members(gpu_device, which, tmp_path):
    from bayesian_inference_for_nn_amd.distributions import Mixture, MultivariateNormalDiagPlusLowRank, Sampled
    from bayesian_inference_for_nn_amd.nn import BayesianModel
    P, n = 3, 20
    step_name, run_name = ENTRY[which]
    a, b = compiled(which, P), compiled(which, P)
    D = a._D
    assert a._theta.shape == (P, D) and a._plan.max_particles == P
    start = a._theta.cpu().numpy().copy()
    assert len({start[c].tobytes() for c in range(P)}) == P and np.array_equal(start, b._theta.cpu().numpy())
    assert np.array_equal(start[0], starting_model(regression()[1]).weights_flat)       # member 0 copies the starting model
    calls_a, calls_b = count_calls(a, which), count_calls(b, which)
    a.train(n)                                        # quiet: one members run through _run_resident_chunks
    for _ in range(n):
        ret = b.step()
    assert calls_a == {step_name: 0, run_name: 1} and calls_b == {step_name: n, run_name: 0}
    sa, sb = state_of(a, which), state_of(b, which)
    for name in STATE[which]:
        assert np.array_equal(bits(sa[name]), bits(sb[name])), name
    assert a._n == b._n == n and a.last_losses.shape == (n, P)
    losses = a.last_losses.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(losses))
    if which == "SGD":                                # the running mean over the batches of the current epoch
        assert a._seen_batches == b._seen_batches and a._epoch_num == b._epoch_num > 1
        assert float(ret) == pytest.approx(losses[n - a._seen_batches:].mean(), rel=1e-5)
        assert float(a._running_dev.item()) == pytest.approx(float(b._running_dev.item()), rel=1e-5)
    else:
        assert a._n_cols == b._n_cols == 3
        assert float(ret) == pytest.approx(losses[-1].mean(), rel=1e-5)
    theta, mean = sa["_theta"], sa["_mean_dev"]
    slices = a._spec.layer_slices()
    # member_results(): per member what result() of a single optimizer builds from that row
    members = a.member_results()
    assert len(members) == P
    for c, m in enumerate(members):
        assert np.array_equal(m._model.weights_flat, theta[c]) and len(m._distributions) == len(slices)
        for li, sl in enumerate(slices):
            d = m._distributions[li]
            if which == "SGD":
                assert np.array_equal(bits(d._tf_distribution.loc), bits(mean[c][sl]))
            else:
                assert isinstance(d, MultivariateNormalDiagPlusLowRank)
                for gotp, want in zip((d._mean, d._diag, d._D), lowrank_params(a, mean[c], sa["_sq_mean_dev"][c], sa["_dev_rows"][c], sl)):
                    assert np.array_equal(bits(gotp), bits(want))
    # result(): ONE distribution over all layers, the members' rows bit for bit; the net's weights are member 0's
    res = a.result()
    assert res._layers_dtbn_intervals == [[0, len(a._net.layers) - 1]] and len(res._distributions) == 1
    assert np.array_equal(res._model.weights_flat, theta[0])

    def check_dist(dist):
        if which == "SGD":
            assert isinstance(dist, Sampled) and dist._frequencies == [1] * P and dist.size == D
            for c in range(P):
                assert np.array_equal(bits(dist._samples[c]), bits(mean[c]))
        else:
            assert isinstance(dist, Mixture) and dist._frequencies == [1] * P and dist.size == D
            for c, comp in enumerate(dist.components):
                assert isinstance(comp, MultivariateNormalDiagPlusLowRank) and comp._D.shape == (D, 3)
                for gotp, want in zip((comp._mean, comp._diag, comp._D), lowrank_params(a, mean[c], sa["_sq_mean_dev"][c], sa["_dev_rows"][c])):
                    assert np.array_equal(bits(gotp), bits(want))
    check_dist(res._distributions[0])
    x = np.linspace(-1.0, 1.0, 9, dtype=np.float32).reshape(9, 1)
    samples, mean_pred = res.predict(x, 16)
    assert len(samples) == 16 and all(np.asarray(s).shape == (9, 1) for s in samples) and np.asarray(mean_pred).shape == (9, 1)
    assert np.all(np.isfinite(np.asarray(samples))) and np.all(np.isfinite(np.asarray(mean_pred)))
    res.store(str(tmp_path / "model"))
    back = BayesianModel.load(str(tmp_path / "model"))
    assert back._layers_dtbn_intervals == res._layers_dtbn_intervals
    check_dist(back._distributions[0])
    if which == "SGD":                                # the MultiSWAG recipe: SWAG's member c starts at SGD's member c
        models = a.member_models()
        assert len(models) == P and all(np.array_equal(models[c].weights_flat, theta[c]) for c in range(P))
        multi = compiled("SWAG", P, start=models)
        assert np.array_equal(bits(multi._theta.cpu().numpy()), bits(theta))
        with pytest.raises(ValueError):
            compiled("SWAG", P, start=models[:2])


@pytest.mark.parametrize("which", ["SGD", "SWAG"])
def test_member_zero_follows_the_one_member_optimizer(gpu_device, which):
    """Same seed and starting model: member 0 starts where the one-member optimizer starts and sees the same batches; its
    gradients come from the particle-batched pass instead of the fused single-model step, so after three steps the two
    agree block by block within the bound of compare_step's increments, not bit for bit.  The one-member optimizer
    (n_members = 1, and no kwarg at all) never reaches the new entry points, and the two stay bit-equal."""
    three, one, default = compiled(which, 3), compiled(which, 1), compiled(which, None)
    calls_one, calls_default = count_calls(one, which), count_calls(default, which)
    start = one._theta.cpu().numpy().copy()
    assert one._theta.shape == (one._D,) and np.array_equal(start, three._theta.cpu().numpy()[0])
    assert np.array_equal(start, default._theta.cpu().numpy())
    for opt in (three, one, default):
        for _ in range(3):
            opt.step()
    got, ref = three._theta.cpu().numpy()[0].astype(np.float64), one._theta.cpu().numpy().astype(np.float64)
    from oracle import mlp as o_mlp
    spec = o_mlp.MLPSpec((1, 5, 1), ("tanh", "linear"), "mse")
    close_blocks(got - start, ref - start, spec, what="member 0 against the one-member optimizer",
                 state=np.maximum(np.abs(got), np.abs(start)))
    one.train(4)
    default.train(4)
    for name in STATE[which]:
        assert np.array_equal(bits(getattr(one, name).cpu().numpy()), bits(getattr(default, name).cpu().numpy())), name
    assert calls_one == calls_default == {name: 0 for name in ENTRY[which]}
    assert isinstance(one.member_results(), list) and len(one.member_results()) == 1
    assert len(one.result()._distributions) == len(one._spec.layer_slices())          # the per-layer result of today


# ---------------------------------------------------------------- Mixture on the device
def test_mixture_read_out_on_the_device_and_on_the_host(gpu_device, monkeypatch):
    from bayesian_inference_for_nn_amd.distributions import Mixture, MultivariateNormalDiagPlusLowRank
    from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json
    cfg = sequential_json(2, [3, 2], ["tanh", "softmax"])
    model = BayesianModel(cfg)
    D = model._model.spec.n_params
    comps = [MultivariateNormalDiagPlusLowRank(np.full(D, m, dtype=np.float32), np.full(D, 1e-3, dtype=np.float32),
                                               np.zeros((D, 2), dtype=np.float32)) for m in (-100.0, 100.0)]
    mix = Mixture(comps, [1, 2])
    model.apply_distribution(mix, 0, len(model._model.layers) - 1)
    seen = {}
    for device in ("1", "0"):
        monkeypatch.setenv("PYZ_SAMPLE_DEVICE", device)
        random.seed(23)
        W = model.sample_weights_device(64)
        assert W.is_cuda and tuple(W.shape) == (64, D)
        W = W.cpu().numpy()
        random.seed(23)
        idx = [mix.sample_index() for _ in range(64)]
        assert 0 < sum(idx) < 64
        for r, c in enumerate(idx):
            assert np.all(np.abs(W[r] - (-100.0, 100.0)[c]) < 0.1), (device, r, c, W[r])
        counts = [int((W[:, 0] < 0).sum()), int((W[:, 0] > 0).sum())]
        assert counts == [idx.count(0), idx.count(1)]
        seen[device] = W[:, 0] > 0
    assert np.array_equal(seen["1"], seen["0"])       # the host path gives the same assignment
