"""SGLD with P chains per launch on the device: pyz_sgld_chains_step against the float64 restatement
(tests/sgld_chains_checks.py lists the cases), no cross-talk between the rows, pyz_sgld_chains_run against the step calls bit
for bit, and the SGLD surface with n_chains.

A step test is one case: three consecutive steps from n0 = 3 per noise variant.  Before every step the state is read back
and the reference restarts from it, so every bound is step_cases.compare_step's bound on one step of one chain."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bce_checks  # noqa: E402
import sgld_chains_checks as cc  # noqa: E402
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
    """A (P, D) float32 matrix as a view into a sentinel-filled buffer: one element in front (the matrix then starts 4
    bytes off 16-byte alignment) or four (aligned), 64 behind."""

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

    def __init__(self, eng, case, data, P=None):
        self.case, st = case, case.step
        self.P = case.P if P is None else P
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

    def step(self, k, noise, seed=None):
        st, b = self.case.step, self.bufs
        z = None
        if noise is not None:
            self.noise.t.copy_(noise if isinstance(noise, torch.Tensor) else dev(noise))
            z = self.noise.t
        self.loss.t.zero_()
        self.plan.sgld_chains_step(b["theta"].t, b["mean"].t, b["sq"].t, self.x, self.y, st.lr, st.n0 + k,
                                   st.seed if seed is None else seed, self.loss.t, batch=st.batch, row_idx=self.rid,
                                   unit_noise=z)
        got = self.get_state()
        got["loss"] = self.loss.get()
        return got


@pytest.mark.parametrize("case", cc.CASES, ids=[c.name for c in cc.CASES])
def test_step_case(eng, case):
    data = cc.chains_data(case)
    run = Run(eng, case, data)
    worst = {}
    for variant in cc.VARIANTS:
        run.set_state(cc.initial_state(data))
        for k in range(cc.N_STEPS):
            what = f"{case.name} {variant} step {k}"
            s0 = run.get_state()
            inj = cc.injected_noise(case, variant, k)
            got = run.step(k, inj)
            ref = cc.ref_chains_step(case, data, variant, k, s0)
            rep = cc.compare_chains_step(case, k, s0, got, ref, what=f"{variant}: ")
            for q, r in sorted(rep.items()):
                print(f"{what}: {q}: error / tolerance {r:.4f}")
                worst[q] = max(worst.get(q, 0.0), r)
            assert run.guards_broken() == [], f"{what}: wrote outside {run.guards_broken()}"
            # the same step from the same state: the same bits
            run.set_state(s0)
            assert same_bits(got, run.step(k, inj)), f"{what}: repeating the step from the same state gives other bits"
            # the device's own draws are, row by row, the Philox streams of seed + c as fill_normal writes them
            if variant == "device":
                z = torch.stack([eng.fill_normal(torch.empty(case.D, device="cuda"), case.step.seed + c, sc.STREAM["sgld"],
                                                 case.step.n0 + k) for c in range(case.P)])
                run.set_state(s0)
                assert same_bits(got, run.step(k, z)), f"{what}: device noise and the injected streams give different bits"
            assert run.guards_broken() == [], f"{what}: wrote outside {run.guards_broken()}"
    print(f"CASE | {case.name} | " + " | ".join(f"{q} {r:.4f}" for q, r in sorted(worst.items())))
    run.plan.close()


CROSS_TALK = ("f_d66_gathered_p5", "u_d165_mse_p5")


@pytest.mark.parametrize("name", CROSS_TALK)
def test_no_cross_talk_between_chains(eng, name):
    """Row c of a P = 5 step depends on row c of the state and on seed + c alone.
    (a) With every OTHER row of the state replaced, row c comes out with the same bits (same launch geometry: exact).
    (b) Against a P = 1 call of the same entry point with seed + c from the same start: the update is the same arithmetic,
        the gradient pass picks its kernels from the particle count as well (pyz_pick_waves takes tiles x P, the vector
        paths ask for P == 1 or D % 4 == 0), so the rows agree within compare_step; whether they also agree bit for bit at
        these shapes is printed, not asserted."""
    case = cc.CASE_BY_NAME[name]
    data = cc.chains_data(case)
    s0 = cc.initial_state(data)
    run = Run(eng, case, data)
    one = Run(eng, case, data, P=1)
    k = 1
    for variant in ("philox", "device"):
        inj = cc.injected_noise(case, variant, k)
        run.set_state(s0)
        got = run.step(k, inj)
        ref = cc.ref_chains_step(case, data, variant, k, s0)
        for c in range(case.P):
            # (a)
            other = {key: np.roll(v, 1, axis=0) * np.float32(1.25) for key, v in s0.items()}
            for key in other:
                other[key][c] = s0[key][c]
            run.set_state(other)
            again = run.step(k, inj)
            for key in ("theta", "mean", "sq", "loss"):
                assert np.array_equal(bits(again[key][c]), bits(got[key][c])), f"{name} {variant}: row {c} of {key} moved with the other rows"
            # (b)
            one.set_state({key: v[c:c + 1] for key, v in s0.items()})
            g1 = one.step(k, None if inj is None else inj[c:c + 1], seed=case.step.seed + c)
            g1 = {key: v[0] for key, v in g1.items()}
            sc.compare_step(cc.chain_case(case, c), "sgld", k, cc.chain_state(s0, c), g1, cc.chain_state(ref, c),
                            what=f"P = 1 call, chain {c}: ")
            sc.compare_step(cc.chain_case(case, c), "sgld", k, cc.chain_state(s0, c), cc.chain_state(got, c),
                            {key: np.asarray(v, dtype=np.float64) for key, v in g1.items()}, what=f"row {c} of P = 5 against P = 1: ")
            eq = all(np.array_equal(bits(g1[key]), bits(got[key][c])) for key in g1)
            print(f"BITS | {name} | {variant} | chain {c} | P = 5 row against the P = 1 call: {'equal' if eq else 'different'}")
    assert run.guards_broken() == [] and one.guards_broken() == []
    run.plan.close()
    one.plan.close()


# ---------------------------------------------------------------- the run
RUN_SHAPES = {
    "fused_p3": ((5, 7, 3), ("tanh", "softmax"), "scce", 3),
    "unfused_p2": ((3, 5, 33), ("tanh", "softmax"), "scce", 2),
}


@pytest.mark.parametrize("shape", sorted(RUN_SHAPES))
def test_run_equals_step_calls_bit_for_bit(eng, shape):
    """7 steps with batches 8, 8, 5, 8, 8, 5, 8 over 21 rows (ragged, two epoch changes), then 7 more from slot 7: theta,
    mean, sq_mean and every loss equal the step calls bit for bit, with use_graph 0 and 1."""
    dims, acts, loss, P = RUN_SHAPES[shape]
    spec = eng.MLPSpec(dims, acts, loss)
    D, B, N, seed, n0 = spec.n_params, 8, 21, 29, 3
    rng = np.random.default_rng(5)
    x = dev(rng.normal(size=(N, dims[0])))
    y = dev(rng.integers(0, dims[-1], size=N), torch.int32)
    sizes = ([8, 8, 5] * 5)[:14]                     # epochs of 21 rows; the second call goes on inside the third epoch
    assert tuple(sizes[:7]) == cc.RUN_SIZES
    lrs = cc.run_lrs(14)
    table = np.zeros((14, B), dtype=np.int32)
    s = 0
    while s < 14:                                    # an epoch = a permutation of the 21 rows in batches of 8, 8, 5
        perm, o = rng.permutation(N), 0
        for b in (8, 8, 5):
            if s < 14:
                assert sizes[s] == b
                table[s, :b] = perm[o:o + b]
                o, s = o + b, s + 1
    table_dev = dev(table, torch.int32)
    start = {"theta": (rng.normal(size=(P, D)) * 0.5).astype(np.float32), "mean": rng.normal(size=(P, D)).astype(np.float32),
             "sq": rng.uniform(1.0, 2.0, size=(P, D)).astype(np.float32)}
    plan = eng.MLPPlan(spec, max_batch=B, max_particles=P)

    def fresh():
        return {k: dev(v) for k, v in start.items()}

    st = fresh()
    step_losses = torch.zeros((14, P), device="cuda")
    snap = {}
    for s in range(14):
        plan.sgld_chains_step(st["theta"], st["mean"], st["sq"], x, y, lrs[s], n0 + s, seed, step_losses[s], batch=sizes[s],
                              row_idx=table_dev[s, :sizes[s]])
        if s in (6, 13):
            snap[s] = {k: v.cpu().numpy().copy() for k, v in st.items()}
    step_losses = step_losses.cpu().numpy()
    assert np.all(np.isfinite(step_losses)) and len({step_losses[0, c].tobytes() for c in range(P)}) == P
    for use_graph in (False, True):
        rt = fresh()
        losses = torch.full((14, P), SENTINEL, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            plan.sgld_chains_run(rt["theta"], rt["mean"], rt["sq"], x, y, table_dev, sizes[:7], lrs[:7], n0, seed, losses,
                                 use_graph=use_graph)
            kind, steps = plan.last_run_path()
            assert steps == 7 and kind in ("graph", "eager", "mixed")
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in rt.items()}
        lo = losses.cpu().numpy()
        for k in got:
            assert np.array_equal(bits(got[k]), bits(snap[6][k])), f"{shape} use_graph={use_graph}: {k} after 7 steps"
        assert np.array_equal(bits(lo[:7]), bits(step_losses[:7])) and np.all(lo[7:] == SENTINEL)
        with torch.cuda.stream(stream):             # ... and on from slot 7
            plan.sgld_chains_run(rt["theta"], rt["mean"], rt["sq"], x, y, table_dev, sizes[7:], lrs[7:], n0 + 7, seed, losses,
                                 use_graph=use_graph, slot0=7)
            assert plan.last_run_path()[1] == 7
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in rt.items()}
        for k in got:
            assert np.array_equal(bits(got[k]), bits(snap[13][k])), f"{shape} use_graph={use_graph}: {k} after 14 steps"
        assert np.array_equal(bits(losses.cpu().numpy()), bits(step_losses))
    plan.check_finite()
    plan.close()


def test_shape_errors(eng):
    from bayesian_inference_for_nn_amd._lib import PyzError, check, ptr
    spec = eng.MLPSpec((3, 4, 2), ("tanh", "softmax"), "scce")
    plan = eng.MLPPlan(spec, max_batch=8, max_particles=2)
    D = spec.n_params
    th = torch.zeros((3, D), device="cuda")
    x, y, lo = torch.zeros((8, 3), device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(3, device="cuda")
    for batch, P in ((8, 3), (9, 2)):                 # more chains than the plan's particles; a batch outside the plan
        rc = plan.lib.pyz_sgld_chains_step(plan.h, ptr(th), ptr(th), ptr(th), P, ptr(x), ptr(y), None, batch, 0.1, 0, 1, None,
                                           ptr(lo), None)
        assert rc == -2                               # PYZ_E_SHAPE
        with pytest.raises(PyzError):
            check(rc)
    plan.close()


# ---------------------------------------------------------------- the SGLD surface
def regression():
    from bayesian_inference_for_nn_amd import synth
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import MeanSquaredError
    from bayesian_inference_for_nn_amd.nn import sequential_json
    x, y = synth.linreg(70)
    x, y = x / 20.0, y / 40.0
    return Dataset((x, y), MeanSquaredError, "Regression", seed=0), sequential_json(1, [5, 1], ["tanh", "linear"])


def compiled(n_chains, seed=17, **kw):
    from bayesian_inference_for_nn_amd.optimizers import SGLD
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    ds, cfg = regression()
    opt = SGLD()
    extra = {} if n_chains is None else {"n_chains": n_chains}
    opt.compile(HyperParameters(lr_upper=0.02, lr_lower=0.005, lr_gamma=0.9, batch_size=16), cfg, ds, verbose=False, seed=seed,
                **extra, **kw)
    return opt


def count_calls(opt):
    """Counting wrappers on the plan's two new methods."""
    calls = {"sgld_chains_step": 0, "sgld_chains_run": 0}
    for name in calls:
        inner = getattr(opt._plan, name)

        def wrapper(*a, _inner=inner, _name=name, **kw):
            calls[_name] += 1
            return _inner(*a, **kw)
        setattr(opt._plan, name, wrapper)
    return calls


def test_surface_with_three_chains(gpu_device):
    from bayesian_inference_for_nn_amd.optimizers.SGLD import pool_chain_moments
    P, n = 3, 20
    a, b = compiled(P), compiled(P)
    D = a._D
    assert a._theta.shape == (P, D) and a._plan.max_particles == P
    start = a._theta.cpu().numpy().copy()
    assert len({start[c].tobytes() for c in range(P)}) == P and np.array_equal(start, b._theta.cpu().numpy())
    calls_a, calls_b = count_calls(a), count_calls(b)
    a.train(n)                                        # quiet: pyz_sgld_chains_run through _run_resident_chunks
    b._nb_iterations = n
    b._init_sgld_lr()
    for _ in range(n):
        ret = b.step()
    assert calls_a == {"sgld_chains_step": 0, "sgld_chains_run": 1} and calls_b == {"sgld_chains_step": n, "sgld_chains_run": 0}
    for name in ("_theta", "_mean_dev", "_sq_mean_dev"):
        assert np.array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy())), name
    assert a._n == b._n == n and a.last_losses.shape == (n, P)
    assert float(ret) == pytest.approx(float(a._running_dev.item()) / n, rel=1e-5)
    assert float(ret) == pytest.approx(float(a.last_losses.cpu().numpy().astype(np.float64).mean()), rel=1e-5)
    # result(): the float64 average of the chains' moments; the net's weights are chain 0's
    chains = a.chain_results()
    assert len(chains) == P
    pooled = a.result()
    mean, sq = a._mean_dev.cpu().numpy(), a._sq_mean_dev.cpu().numpy()
    m64, s64 = pool_chain_moments(mean, sq)
    m32, s32 = m64.astype(np.float32), s64.astype(np.float32)
    for li, sl in enumerate(a._spec.layer_slices()):
        d = pooled._distributions[li]._tf_distribution
        locs = np.stack([np.asarray(ch._distributions[li]._tf_distribution.loc, dtype=np.float64) for ch in chains])
        assert np.array_equal(np.asarray(d.loc), (locs.sum(axis=0) / P).astype(np.float32))
        assert np.array_equal(np.asarray(d.loc), m32[sl]) and np.array_equal(np.asarray(d.scale), s32[sl] - m32[sl] ** 2)
        for c, ch in enumerate(chains):
            dc = ch._distributions[li]._tf_distribution
            assert np.array_equal(np.asarray(dc.loc), mean[c][sl]) and np.array_equal(np.asarray(dc.scale), sq[c][sl] - mean[c][sl] ** 2)
    theta = a._theta.cpu().numpy()
    assert np.array_equal(pooled._model.weights_flat, theta[0])
    for c, ch in enumerate(chains):
        assert np.array_equal(ch._model.weights_flat, theta[c])
    r = a.r_hat()
    assert r.shape == (D,) and r.dtype == np.float64 and np.all(np.isfinite(r))


def test_chain_zero_follows_the_one_chain_optimizer(gpu_device):
    """Same seed: chain 0 starts where the one-chain optimizer starts, sees the same batches and draws the same noise;
    its gradients come from the particle-batched pass instead of the fused single-chain step, so after three steps the
    two agree block by block within the bound of compare_step's increments, not bit for bit.  The one-chain optimizer
    (n_chains = 1, and no kwarg at all) never reaches the new entry points."""
    three, one, default = compiled(3), compiled(1), compiled(None)
    calls_one, calls_default = count_calls(one), count_calls(default)
    start = one._theta.cpu().numpy().copy()
    assert one._theta.shape == (one._D,) and np.array_equal(start, three._theta.cpu().numpy()[0])
    assert np.array_equal(start, default._theta.cpu().numpy())
    for opt in (three, one, default):
        opt._nb_iterations = 3
        opt._init_sgld_lr()
        for _ in range(3):
            opt.step()
    got, ref = three._theta.cpu().numpy()[0].astype(np.float64), one._theta.cpu().numpy().astype(np.float64)
    from oracle import mlp as o_mlp
    spec = o_mlp.MLPSpec((1, 5, 1), ("tanh", "linear"), "mse")
    close_blocks(got - start, ref - start, spec, what="chain 0 against the one-chain optimizer",
                 state=np.maximum(np.abs(got), np.abs(start)))
    assert np.array_equal(bits(one._theta.cpu().numpy()), bits(default._theta.cpu().numpy()))
    one.train(4)
    default.train(4)
    assert calls_one == calls_default == {"sgld_chains_step": 0, "sgld_chains_run": 0}
    assert isinstance(one.chain_results(), list) and len(one.chain_results()) == 1
    with pytest.raises(ValueError):
        one.r_hat()
