"""BinaryCrossentropy on the device, through every path that reaches a loss head, against the float64 restatement of
tests/bce_checks.py: the head matrix (k_head_rows<UT, 4, RW>, k_head), one eager step and one short device-resident run of
SGD, SWAG, SGLD, BBB, ADAM, VADAM and BSAM, an SVGD step of either sweep, the four HMC paths, pyz_input_grad / FGSM, and
the reference's one-sigmoid-output flow on the drop-in surface.

The steps, runs and HMC proposals go through the drivers and the comparisons of the existing matrix tests unchanged
(test_gpu_step_matrix.Run, test_gpu_run_matrix.Dev / per_step, test_gpu_adam_bsam_run.Case, test_gpu_hmc_matrix.Runner,
step_cases.compare_step, run_cases.compare_run_step, hmc_cases.compare): bce_checks.install puts the BCE loss under the
oracle's step functions for the length of a test.  Bounds: head_cases.close_blocks for gradients, 1e-4 relative for losses,
and whatever those comparisons apply to their MSE cases."""

import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bce_checks as bc  # noqa: E402
import hmc_cases as hc  # noqa: E402
import run_cases as rc  # noqa: E402
import step_cases as sc  # noqa: E402
import test_gpu_adam_bsam_run as tab  # noqa: E402
import test_gpu_hmc_matrix as thm  # noqa: E402
import test_gpu_run_matrix as trm  # noqa: E402
import test_gpu_step_matrix as tsm  # noqa: E402
from adam_checks import AdamRef, epoch_plan  # noqa: E402
from bsam_checks import BsamRef  # noqa: E402
from head_cases import check_particles, close_blocks, expected_head_kernel  # noqa: E402
from input_grad_checks import fgsm  # noqa: E402
from oracle import mlp as o_mlp  # noqa: E402
from oracle import philox as o_philox  # noqa: E402

DIMS, ACTS = (2, 8, 1), ("tanh", "sigmoid")      # the small model of the step, run, SVGD, HMC and FGSM tests
ROWS, BATCH, RUN_SIZES = 80, 32, (32, 32, 16, 32, 32)


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in rc.ENV_FORBIDDEN if os.environ.get(k)] + sorted(k for k in os.environ if k.startswith("PYZ_HMC_"))
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the expected kernels of this module assume the defaults")
    from bayesian_inference_for_nn_amd import engine
    return engine


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def loss_close(v, ref, what):
    assert np.isfinite(v), f"{what}: {v!r}"
    assert abs(float(v) - ref) <= 1e-4 * abs(ref), f"{what}: {float(v)!r} vs {ref!r}"


# ---------------------------------------------------------------- the head matrix
@pytest.mark.parametrize("case", bc.HEAD_CASES, ids=[c.name for c in bc.HEAD_CASES])
def test_head_case(eng, case):
    spec, P, B = case.spec, case.P, case.batch
    x, y, idx, thetas = bc.case_data(case)
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, "bce"), max_batch=B + 5, max_particles=P)
    xd = tsm.dev(x)
    if case.extra.get("x_offset"):
        buf = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
        buf[1:].copy_(dev(x).reshape(-1))
        xd = buf[1:].view(x.shape)
        assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    yd, th = dev(y), dev(thetas)
    rid = dev(idx, torch.int32) if idx is not None else None
    with eng.KernelProbe(32) as kp:
        loss, grad = plan.loss_grad(th, xd, yd, batch=B, row_idx=rid)
    names = [n.replace(" ", "") for n, _ in kp.launches]
    kernel = expected_head_kernel(case.dims, "mse", P, B)      # the dispatch does not depend on the loss
    assert kernel.replace(" ", "") in names, (kernel, kp.launches)
    assert not any(n.startswith("k_loss_") and n != "k_loss_finalize" for n in names), names
    out = plan.forward(th, xd, batch=B, row_idx=rid)
    loss_only, none = plan.loss_grad(th, xd, yd, batch=B, row_idx=rid, want_grad=False)
    assert none is None
    plan.check_finite()
    loss, loss_only = loss.cpu().numpy(), loss_only.cpu().numpy()
    rows, ys = (x, y) if idx is None else (x[idx], y[idx])
    for p in check_particles(P):
        rl, rg, rout = bc.loss_and_grad(thetas[p], rows, ys, spec)
        loss_close(loss[p], rl, f"{case.name} loss[{p}]")
        loss_close(loss_only[p], rl, f"{case.name} loss only[{p}]")
        close_blocks(grad[p], rg, spec, what=f"{case.name} grad[{p}]")
        o = out[p].cpu().numpy().astype(np.float64)
        assert o.shape == rout.shape and np.all(np.isfinite(o))
        assert np.abs(o - rout).max() <= 1e-4 * np.abs(rout).max(), f"{case.name} output[{p}]"
    plan.close()


# ---------------------------------------------------------------- SGD, SWAG, SGLD, BBB: one eager step
@pytest.mark.parametrize("mode", sc.MODES)
def test_eager_step(eng, monkeypatch, mode):
    bc.install(monkeypatch)
    case = sc.StepCase("bce_step", DIMS, ACTS, "bce", BATCH, gathered=True)
    data = sc.step_data(case)
    assert data.y.dtype == np.float32 and data.y.shape[1] == 1 and 0.0 <= data.y.min() and data.y.max() <= 1.0
    run = tsm.Run(eng, case, mode, data)
    variant = "device" if mode in sc.STREAM else "plain"
    s0 = run.get_state()
    got = run.step(0, None)
    ref = sc.ref_step(case, data, mode, variant, 0, s0)
    for q, r in sorted(sc.compare_step(case, mode, 0, s0, got, ref).items()):
        print(f"bce {mode} step: {q}: error / tolerance {r:.4f}")
    assert run.guards_intact() == []
    run.plan.check_finite()
    run.plan.close()


# ---------------------------------------------------------------- SGD, SWAG, SGLD, BBB: one short device-resident run
def run_case():
    return rc.RunCase("bce_run", DIMS, ACTS, "bce", BATCH, RUN_SIZES, n0=8)     # n = 8 .. 12: BBB's gate closes at n = 10


def run_data(case):
    """run_cases.run_data with the data set grown to 80 rows (the added ones carry 0 / 1 labels), a row table over all of
    them and validation targets in [0, 1]."""
    d = rc.run_data(case, slots=12)
    rng = np.random.default_rng(97)
    extra = ROWS - len(d.step.x)
    x = np.concatenate([d.step.x, rng.normal(size=(extra, DIMS[0])).astype(np.float32)])
    y = np.concatenate([d.step.y, rng.integers(0, 2, size=(extra, 1)).astype(np.float32)])
    tab_ = np.stack([rng.permutation(ROWS)[:case.max_batch] for _ in range(12)]).astype(np.int32)
    yv = rng.uniform(0.0, 1.0, size=(rc.N_VAL, 1)).astype(np.float32)
    return d._replace(step=d.step._replace(x=x, y=y), tab=tab_, yv=yv)


@pytest.mark.parametrize("mode", sc.MODES)
def test_resident_run(eng, monkeypatch, mode):
    """Five steps, the third on the ragged batch of 16: every step against the oracle restarted from the state before it,
    the graph replay against the eager-chained run (test_gpu_run_matrix.per_step), then the run against the same steps as
    eager *_step calls: bit for bit with whole batches, 2e-6 of the largest magnitude with the ragged one (the chain tier's
    claim)."""
    bc.install(monkeypatch)
    case = run_case()
    data = run_data(case)
    val = mode == "bbb"
    call = case.call(mode, len(RUN_SIZES), val=val)
    assert call.sizes == RUN_SIZES and (not val or [(call.n0 + i) % rc.GATE_MOD != 0 for i in range(5)] == [True, True, False, True, True])
    d = trm.Dev(eng, case, mode, data, slots=12, val=val)
    start = rc.initial_state(mode, data, call.k)
    trm.per_step(d, case, data, call, mode, start, f"bce {mode}")
    for sizes, exact in ((RUN_SIZES, False), ((BATCH,) * 5, True)):
        c = call._replace(sizes=sizes, lrs=tuple(lr / 64 for lr in call.lrs))      # (the chain tier's learning rates)
        d.reset(start)
        d.eager(c)
        want = (d.state(), d.outputs())
        d.reset(start)
        d.run(c, use_graph=True)
        trm.assert_same((d.state(), d.outputs()), want, f"bce {mode} run against the step loop, batches {sizes}", exact=exact)
        assert d.guards() == []
    d.plan.check_finite()
    d.close()


# ---------------------------------------------------------------- ADAM, VADAM, BSAM
def adam_case(eng):
    """test_gpu_adam_bsam_run.Case on the BCE model: 80 rows in batches of 32, 32 and 16."""
    c = tab.Case.__new__(tab.Case)
    c.spec, c.n, c.batch = bc.spec(DIMS, ACTS), ROWS, BATCH
    rng = np.random.default_rng(23)
    c.x = rng.normal(size=(ROWS, DIMS[0])).astype(np.float32)
    c.y = np.where(rng.uniform(size=(ROWS, 1)) < 0.5, rng.integers(0, 2, size=(ROWS, 1)), rng.uniform(size=(ROWS, 1))).astype(np.float32)
    c.theta0 = (rng.normal(size=c.spec.n_params) * 0.3).astype(np.float32)
    c.plan = eng.MLPPlan(eng.MLPSpec(DIMS, ACTS, "bce"), max_batch=BATCH)
    c.xd, c.yd, c.D = dev(c.x), dev(c.y), c.spec.n_params
    c.batches = epoch_plan(ROWS, BATCH, 5, seed=3)
    c.idx_dev = [dev(i, torch.int32) for i, _ in c.batches]
    assert [len(i) for i, _ in c.batches] == list(RUN_SIZES)
    return c


def adam_reference(c, kind, count):
    """test_run_matches_the_float64_restatement's loop."""
    ref = BsamRef(c.theta0) if kind == "bsam" else AdamRef(c.theta0)
    want = []
    for i, (idx, epoch) in enumerate(c.batches[:count]):
        if kind == "bsam":
            want += list(ref.step(c.x[idx], c.y[idx], c.spec, o_philox.normal(tab.SEED, 6, i, c.D), num_data=float(c.n), **tab.BSAM_HYP))
        elif kind == "vadam":
            ref.perturb(o_philox.normal(tab.SEED, 5, i, c.D), tab.LAM, float(c.n))
            want.append(ref.step(c.x[idx], c.y[idx], c.spec, tab.LR, tab.B1, tab.B2, epoch, denom_eps=tab.LAM / c.n, decay=tab.LAM / c.n))
        else:
            want.append(ref.step(c.x[idx], c.y[idx], c.spec, tab.LR, tab.B1, tab.B2, epoch))
    return ref, want


@pytest.mark.parametrize("kind", tab.KINDS)
def test_adam_family_step_and_run(eng, monkeypatch, kind):
    """One eager step and a run of five against the float64 restatements (1e-4 of the largest reference magnitude, the
    bound of tests/test_gpu_adam_bsam_run.py), and the run against five eager steps, bit for bit."""
    bc.install(monkeypatch)
    c, k = adam_case(eng), tab.per_step(kind)
    for count in (1, 5):
        st = c.state(kind)
        losses = torch.zeros(k * count, device="cuda")
        if count == 1:
            c.eager(kind, st, 0, 1, 0, losses)
            c.plan.check_finite()
        else:
            c.run(kind, st, 0, count, 0, losses)
            assert c.plan.last_run_path() == ("graph", count)
        ref, want = adam_reference(c, kind, count)
        th, m, v = tab.host(st)
        what = f"bce {kind} {'step' if count == 1 else 'run'}"
        tab.close(losses.cpu().numpy(), want, what=f"{what} losses")
        tab.close(th, ref.theta, what=f"{what} theta")
        tab.close(m, ref.m, what=f"{what} m")
        tab.close(v, ref.v, what=f"{what} v")
    loop = c.state(kind)
    loop_losses = torch.zeros(k * 5, device="cuda")
    c.eager(kind, loop, 0, 5, 0, loop_losses)
    tab.assert_same(tab.host(st), losses.cpu().numpy(), tab.host(loop), loop_losses.cpu().numpy(), f"bce {kind} run against the step loop")
    c.plan.close()


# ---------------------------------------------------------------- SVGD
@pytest.mark.parametrize("sweep", ["gauss_seidel", "jacobi"])
def test_svgd_step(eng, monkeypatch, sweep):
    """tests/test_gpu_parity.py::test_svgd_step_matches_oracle on the BCE model with four particles, one step."""
    bc.install(monkeypatch)
    from oracle import svgd as o_svgd
    spec = o_mlp.MLPSpec(DIMS, ACTS, "bce")
    rng = np.random.default_rng(61)
    x = rng.normal(size=(ROWS, DIMS[0])).astype(np.float32)
    y = rng.integers(0, 2, size=(ROWS, 1)).astype(np.float32)
    M, D = 4, spec.n_params
    parts = (rng.normal(size=(M, D)) * 0.15).astype(np.float32)       # close together: K far from I
    st = o_svgd.SVGDState(parts)
    plan = eng.MLPPlan(eng.MLPSpec(DIMS, ACTS, "bce"), max_batch=ROWS, max_particles=M)
    p = dev(parts)
    am, av = torch.zeros((M, D), device="cuda"), torch.zeros((M, D), device="cuda")
    loss = torch.zeros(1, device="cuda")
    plan.svgd_step(p, p.clone() if sweep == "jacobi" else p, 0, am, av, dev(x), dev(y), 0.05, 1.0, 1, loss, sweep=sweep)
    out = o_svgd.svgd_step(st, x, y, spec, 0.05, 1.0, sweep=sweep)
    plan.check_finite()
    tab.close(loss.cpu().numpy(), [out["loss"]], what=f"bce svgd {sweep} loss")
    tab.close(p.cpu().numpy(), st.particles, rel=2e-4, what=f"bce svgd {sweep} particles")
    tab.close(am.cpu().numpy(), st.m, rel=2e-4, what=f"bce svgd {sweep} adam m")
    plan.close()


# ---------------------------------------------------------------- HMC
HMC = [  # name, dims, acts, rows, per-call switches, the path
    ("bce_fused", DIMS, ACTS, 64, {}, "fused"),
    ("bce_multi", DIMS, ACTS, 200, hc.NO_RES, "multi"),
    ("bce_resident", DIMS, ACTS, 200, {}, "resident"),
    ("bce_generic", (2, 6, 5, 1), ("tanh", "relu", "sigmoid"), 50, {}, "generic"),
]


@pytest.mark.parametrize("name,dims,acts,rows,env,path", HMC, ids=[h[0] for h in HMC])
def test_hmc_path(eng, monkeypatch, name, dims, acts, rows, env, path):
    """Two chains, three leapfrog steps: the launches of the path, then energies, decisions and q against oracle.hmc with
    hmc_cases.compare.  Tolerances by hmc_cases' rule, from the float32 oracle's own error on these inputs."""
    bc.install(monkeypatch)
    case = hc._c(name, dims, acts, "bce", rows, 2, 3, 0.05, env=env)
    thm.set_env(monkeypatch, case)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    pa = hc.dispatch(dims, acts, "mse", rows, case.P, case.L, False, case.env, cu)
    assert pa.path == path
    data = hc.case_data(case)
    data = data._replace(y=np.clip(data.y, 0.0, 1.0).astype(np.float32))          # the model's own output plus noise, as targets
    us = []
    for c in range(case.P):                                                      # hmc_cases._uniforms: chain 0 accepted, chain 1 rejected
        ratio = math.exp(min(hc.oracle_result(case, data, c, u=0.5)["log_ratio"], 50.0))
        us.append(float(np.float32(0.5 * ratio if c % 2 == 0 else 2.0 * ratio + 0.1)))
    refs = [hc.oracle_result(case, data, c, u=us[c]) for c in range(case.P)]
    rel32 = hc.measured_rel32(case, [(hc.oracle_result(case, data, c, np.float32, u=us[c]), refs[c]) for c in range(case.P)])
    run = thm.Runner(eng, case, data)
    with eng.KernelProbe(2048) as kp:
        burn = run.call(data.q0, us, True)
    sites = tuple(n for n, _ in kp.launches if n in hc.HMC_SITES)
    assert sites == pa.launches, f"{name}: expected the {pa.path} path {pa.launches}, launched {sites}"
    metro = run.call(data.q0, us, False)
    assert bool((burn[1][:, 0] == 1.0).all())
    for c in range(case.P):
        assert refs[c]["accepted"] == (c % 2 == 0)
        report = hc.compare(thm.chain_result(case, data.q0[c], data.z[c], burn, metro, c), refs[c], case, what=f"chain {c}: ", rel32=rel32)
        thm.note_worst(case, pa.path, report)
    assert run.inputs_unchanged()
    run.close()


# ---------------------------------------------------------------- pyz_input_grad / FGSM
def test_input_grad_and_fgsm(eng):
    """Three draws in chunks of two: the summed input gradient to 1e-4 of its largest entry (tests/test_gpu_input_grad.py),
    the draws' losses to 1e-4, and the FGSM step wherever |gradient| exceeds that bound (there float32 cannot turn the sign)."""
    spec = bc.spec(DIMS, ACTS)
    rng = np.random.default_rng(71)
    n, eps = 45, 0.125
    x = rng.normal(size=(n, DIMS[0])).astype(np.float32)
    y = np.where(rng.uniform(size=(n, 1)) < 0.7, rng.integers(0, 2, size=(n, 1)), rng.uniform(size=(n, 1))).astype(np.float32)
    thetas = (0.5 * rng.normal(size=(3, spec.n_params))).astype(np.float32)
    G, losses = bc.input_grad(thetas, x, y, spec)
    plan = eng.MLPPlan(eng.MLPSpec(DIMS, ACTS, "bce"), max_batch=n, max_particles=2)
    with eng.KernelProbe(64) as kp:
        g, a, l = plan.input_grad(dev(thetas), dev(x), dev(y), epsilon=eps)
    assert [nm for nm, _ in kp.launches].count("k_input_grad") == 2
    plan.check_finite()
    g, a = g.cpu().numpy(), a.cpu().numpy()
    tol = 1e-4 * np.abs(G).max()
    assert np.abs(g.astype(np.float64) - G).max() <= tol
    np.testing.assert_allclose(l.cpu().numpy(), losses, rtol=1e-4)
    keep = np.abs(G) > tol
    assert keep.mean() > 0.97
    assert np.array_equal(np.sign(g)[keep], np.sign(G)[keep])
    np.testing.assert_array_equal(a[keep], fgsm(x, G, eps)[keep])
    assert np.all(np.abs(a - x) <= np.float32(eps) * (1 + 1e-6))
    half, none, _ = plan.input_grad(dev(thetas), dev(x), dev(y), scale=0.5)
    assert none is None and np.array_equal(half.cpu().numpy(), 0.5 * g)
    plan.close()


# ---------------------------------------------------------------- the reference's flow on the drop-in surface
E2E_LR, E2E_STEPS = 0.5, 25   # full-batch gradient descent of the restatement on these blobs: the loss falls at every step


def blobs(n=200, seed=4):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 2, size=n)
    x = (rng.normal(size=(n, 2)) + np.where(y[:, None] == 1, 2.0, -2.0)).astype(np.float32)
    return x, y


def test_binary_classifier_end_to_end(gpu_device, tmp_path):
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import BinaryCrossentropy
    from bayesian_inference_for_nn_amd.nn import BayesianModel, model_from_json, sequential_json
    from bayesian_inference_for_nn_amd.optimizers import SGD
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    from bayesian_inference_for_nn_amd.visualisations import Metrics, Robustness
    x, y = blobs()
    ds = Dataset((x, y), BinaryCrossentropy, "Classification", seed=5)
    xt, yt = ds.training_dataset().as_numpy()
    assert len(xt) == 160
    cfg = sequential_json(2, [8, 1], ["tanh", "sigmoid"])
    start = model_from_json(cfg)
    start.reset_glorot(np.random.default_rng(9))
    # the restatement's descent
    spec = bc.spec(DIMS, ACTS)
    theta, ref_losses = start.weights_flat.astype(np.float64), []
    for _ in range(E2E_STEPS):
        l, g, _ = bc.loss_and_grad(theta, xt, yt, spec)
        ref_losses.append(float(l))
        theta = theta - E2E_LR * g
    assert all(b < a for a, b in zip(ref_losses, ref_losses[1:])), ref_losses
    # the device's
    opt = SGD()
    opt.compile(HyperParameters(lr=E2E_LR, frequency=1, batch_size=len(xt)), cfg, ds, verbose=False, starting_model=start, seed=11)
    opt.train(E2E_STEPS)
    assert opt._plan.last_run_path()[0] == "graph"
    got = opt.last_losses.cpu().numpy()
    print(f"final loss: device {got[-1]!r}, restatement {ref_losses[-1]!r}")
    loss_close(got[0], ref_losses[0], "first loss")
    loss_close(got[-1], ref_losses[-1], "final loss")
    model = opt.result()
    # Metrics reads the one column as [1 - p, p]
    xs, ys = ds.test_data.as_numpy()
    acc = Metrics(model, ds).accuracy(n_boundaries=3, n_samples=100, data_type="test")
    _, mean = model.predict(xs, 3)
    mean = np.asarray(mean, dtype=np.float64).reshape(len(xs), -1)
    assert mean.shape[1] == 1 and np.all((mean >= 0.0) & (mean <= 1.0))
    assert acc == float(((mean[:, 0] > 0.5).astype(int) == np.asarray(ys).reshape(-1)).mean()) * 100
    assert acc >= 90.0                                         # separable blobs
    rob = Robustness(model, ds).adversarial_robustness(epsilon=0.1, nb_samples=3)
    assert 0.0 <= rob <= 100.0
    # a perturbation of 0.1 against blobs four units apart cannot cost the classifier much: the literal argmax over one
    # column would give the share of class 0 instead
    assert rob >= 80.0
    path = str(tmp_path / "model")
    model.store(path)
    again = BayesianModel.load(path)
    _, mean2 = again.predict(xs, 3)
    assert np.array_equal(np.asarray(mean2), np.asarray(model.predict(xs, 3)[1]))
