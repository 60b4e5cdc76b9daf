"""Conv models on the GPU: the stem's kernels (k_conv_fwd, k_conv_wgrad + k_conv_wgrad_reduce, k_conv_dgrad, k_pool_fwd,
k_pool_bwd) and the conv-net entry points against the float64 restatement of tests/conv_checks.py, at the smallest shapes
at which each kernel can still go wrong (the table in conv_checks.CASES: A-T as the feature shipped, H-K for the launch
paths those do not reach -- tests/test_conv_dispatch_table.py ties each to its path), then SGD / SWAG / BayesianModel end to
end.  tests/test_gpu_conv_paths.py holds the paths that need a shape of their own.

Tolerance: 1e-4 of the reference block's largest magnitude, per layer block, for features, loss,
gradient and step increment."""

import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_checks as cc  # noqa: E402
from step_cases import SWAG_STEPS, _moment, _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = [(n, b) for n in cc.ALL for b in cc.CASES[n].batches]
NEW_KERNELS = ("k_conv_fwd", "k_conv_wgrad", "k_conv_wgrad_reduce", "k_conv_dgrad", "k_pool_fwd", "k_pool_bwd", "k_stem_rows")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def guarded(shape, fill=0.0):
    """A float32 device tensor of `shape` with one sentinel float on either side: (view, check())."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2,), fill, dtype=torch.float32, device="cuda")
    buf[0], buf[-1] = 1234.5, -4321.5

    def check(what=""):
        assert float(buf[0]) == 1234.5 and float(buf[-1]) == -4321.5, f"{what}: a sentinel beside the buffer was overwritten"
    return buf[1:-1].view(*shape), check


def upload_x(x, off_by_four=False):
    """x on the device, 16-byte aligned or 4 bytes off."""
    if not off_by_four:
        t = torch.as_tensor(np.array(x, dtype=np.float32)).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(*x.shape)
    t.copy_(torch.as_tensor(np.array(x, dtype=np.float32)))
    assert t.data_ptr() % 16 == 4
    return t


def plan_of(case, batch, particles=1, slack=cc.PLAN_SLACK):      # (the launch arithmetic of conv_checks.reached_cells counts on it)
    from bayesian_inference_for_nn_amd.engine import ConvPlan
    return ConvPlan(case.spec(), max_batch=batch + slack, max_particles=particles)


def run(plan, theta, x, y, idx, batch, grad_out=None, feat_out=None):
    feat = plan.stem_forward(theta, x, batch=batch, row_idx=idx, out=feat_out)
    out = plan.forward(theta, x, batch=batch, row_idx=idx)
    loss, grad = plan.loss_grad(theta, x, y, batch=batch, row_idx=idx, grad_out=grad_out)
    torch.cuda.synchronize()
    return feat, out, loss, grad


def dev_y(d, rows=None):
    y = d.y if rows is None else d.y[rows]
    return torch.as_tensor(np.array(y)).cuda()


# ---------------------------------------------------------------- forward and gradients, one particle
@pytest.mark.parametrize("name,batch", PAIRS)
def test_forward_and_gradients(gpu_device, name, batch):
    from bayesian_inference_for_nn_amd.engine import KernelProbe
    d = cc.make(name, batch)
    case, spec = d.case, d.case.spec()
    ref = cc.reference(name, batch)
    plan = plan_of(case, batch)
    theta = torch.as_tensor(d.theta[0].copy()).cuda()
    idx = torch.as_tensor(d.idx.copy()).cuda()
    x, y = upload_x(d.x), dev_y(d)
    grad_g, grad_ok = guarded((1, plan.D), fill=7.0)
    feat_g, feat_ok = guarded((1, batch, plan.F), fill=7.0)
    with KernelProbe() as kp:
        feat, out, loss, grad = run(plan, theta, x, y, idx, batch, grad_g, feat_g)
    grad_ok(f"{name} gradient"), feat_ok(f"{name} features")
    e = cc.errors(float(loss[0]), grad[0].cpu().numpy(), feat[0].cpu().numpy(), ref, spec)
    e["out"] = cc.rel(out[0].cpu().numpy(), ref[3])
    cc.assert_close(e, f"{name} batch {batch}: rows through row_idx")
    # the launch record: the new kernels ran
    ran = {n.split("<")[0].strip("()") for n, _ in kp.launches}
    want = {"k_conv_fwd", "k_conv_wgrad", "k_conv_wgrad_reduce"}
    if any(op[0] == "pool" for op in case.stem):
        want |= {"k_pool_fwd", "k_pool_bwd"}
    if sum(op[0] == "conv" for op in case.stem) > 1:
        want |= {"k_conv_dgrad"}
    assert want <= ran, (want - ran, ran)
    if sum(op[0] == "conv" for op in case.stem) == 1:
        assert "k_conv_dgrad" not in ran          # not launched for the first conv
    # the repeated call gives the same bits
    first = [bits(t) for t in (feat, out, loss, grad)]
    again = run(plan, theta, x, y, idx, batch, grad_g, feat_g)
    for a, b, what in zip(first, again, ("features", "out", "loss", "grad")):
        assert np.array_equal(a, bits(b)), f"{name}: {what} changed between two calls"
    # NaN in every image outside the batch changes no bit
    x_nan = d.x.copy()
    x_nan[np.setdiff1d(np.arange(len(d.x)), d.idx)] = np.nan
    for a, b, what in zip(first, run(plan, theta, upload_x(x_nan), y, idx, batch), ("features", "out", "loss", "grad")):
        assert np.array_equal(a, bits(b)), f"{name}: {what} depends on an image outside the batch"
    # contiguous rows (no row_idx), 16-byte aligned and 4 bytes off: the same numbers within the bound
    for off in (False, True):
        xc, yc = upload_x(d.x[d.idx], off), dev_y(d, d.idx)
        feat, out, loss, grad = run(plan, theta, xc, yc, None, batch)
        e = cc.errors(float(loss[0]), grad[0].cpu().numpy(), feat[0].cpu().numpy(), ref, spec)
        cc.assert_close(e, f"{name} batch {batch}: contiguous rows{', x 4 bytes off' if off else ''}")
    plan.check_finite()


def test_stem_backward_alone(gpu_device):
    """pyz_stem_backward from a feature gradient of the caller's: the stem's block of case C's gradient when the feature
    gradient is the one the restatement's Dense layer sends down."""
    name, batch = "C", 33
    d = cc.make(name, batch)
    spec = d.case.spec()
    loss, grad_ref, feat_ref, _ = cc.reference(name, batch)
    theta64 = d.theta[0].astype(np.float64)
    f = cc.forward(spec, theta64, d.x[d.idx].astype(np.float64))
    W, _ = cc.unpack(spec, theta64)[-1]
    z = f["dense"][-1]["z"]
    delta = f["out"].copy()
    delta[np.arange(batch), d.y[d.idx]] -= 1.0
    dfeat = (delta / batch) @ W.T                                   # d loss / d features
    plan = plan_of(d.case, batch)
    theta = torch.as_tensor(d.theta[0].copy()).cuda()
    x, idx = upload_x(d.x), torch.as_tensor(d.idx.copy()).cuda()
    feat = plan.stem_forward(theta, x, batch=batch, row_idx=idx)
    g = plan.stem_backward(theta, x, torch.as_tensor(dfeat.astype(np.float32)[None]).cuda(), batch=batch, row_idx=idx)
    assert cc.rel(feat[0].cpu().numpy(), feat_ref) <= cc.TOL
    e = {k: v for k, v in cc.block_errors(np.concatenate([g[0].cpu().numpy(), grad_ref[plan.D_stem:]]), grad_ref, spec).items()}
    cc.assert_close(e, "C: stem_backward alone", tol=cc.TOL)
    assert z.shape == (batch, 4)


# ---------------------------------------------------------------- three particles, isolated from each other
@pytest.mark.parametrize("name", cc.P_CASES)
def test_three_particles_are_isolated(gpu_device, name):
    batch = cc.CASES[name].batches[-1]
    d = cc.make(name, batch)
    spec = d.case.spec()
    plan = plan_of(d.case, batch, particles=3)
    x, y, idx = upload_x(d.x), dev_y(d), torch.as_tensor(d.idx.copy()).cuda()
    theta = torch.as_tensor(d.theta.copy()).cuda()
    grad_g, grad_ok = guarded((3, plan.D), fill=7.0)
    feat, out, loss, grad = run(plan, theta, x, y, idx, batch, grad_g)
    grad_ok(f"{name} gradient of three particles")
    for p in range(3):
        ref = cc.reference(name, batch, p)
        e = cc.errors(float(loss[p]), grad[p].cpu().numpy(), feat[p].cpu().numpy(), ref, spec)
        e["out"] = cc.rel(out[p].cpu().numpy(), ref[3])
        cc.assert_close(e, f"{name} batch {batch} particle {p} of 3")
    clean = [bits(t) for t in (feat, out, loss, grad)]
    theta_nan = d.theta.copy()
    theta_nan[1] = np.nan
    got = run(plan, torch.as_tensor(theta_nan).cuda(), x, y, idx, batch)
    for a, b, what in zip(clean, got, ("features", "out", "loss", "grad")):
        b = bits(b)
        for p in (0, 2):
            assert np.array_equal(a[p], b[p]), f"{name}: {what} of particle {p} changed when particle 1 became NaN"
    assert torch.isnan(got[2][1])


# ---------------------------------------------------------------- steps
def close_increment(got1, s0, ref1, spec, what):
    """theta1 - theta0 against the reference increment per block: TOL of the block's reference scale, plus 2^-23 of the
    block's largest |state| for the two float32 roundings of what is stored (the rule of tests/step_cases.py)."""
    a0 = s0.astype(np.float64)
    inc, ref = got1.astype(np.float64) - a0, ref1 - a0
    rep = {}
    for li, sl in enumerate(spec.layer_slices()):
        ks = spec.variable_shapes()[li][0]
        n = int(np.prod(ks))
        for nm, s in ((f"W{li}", slice(sl.start, sl.start + n)), (f"b{li}", slice(sl.start + n, sl.stop))):
            tol = cc.TOL * np.abs(ref[s]).max() + 2.0 ** -23 * max(np.abs(a0[s]).max(), np.abs(got1[s]).max())
            rep[nm] = float(np.abs(inc[s] - ref[s]).max() / tol)
    print(what, {k: f"{v:.2e}" for k, v in rep.items()})
    bad = {k: v for k, v in rep.items() if not v <= 1.0}
    assert not bad, f"{what}: increments beyond the tolerance (in units of it): {bad}"


@pytest.mark.parametrize("name", cc.ALL)
def test_sgd_step_and_three_chained_swag_steps(gpu_device, name):
    batch = cc.CASES[name].batches[-1]
    d = cc.make(name, batch)
    spec = d.case.spec()
    plan = plan_of(d.case, batch)
    x, y, idx = upload_x(d.x), dev_y(d), torch.as_tensor(d.idx.copy()).cuda()
    xb, yb = d.x[d.idx].astype(np.float64), d.y[d.idx]
    # the largest learning rate whose float64 chain stays off the ties and keeps every block's gradient alive (cc.step_lr);
    # the device's own chained states are held to the generator's margin below
    lr, D = cc.step_lr(name, batch), plan.D
    ref_loss, ref_grad, _, _ = cc.reference(name, batch)
    # one SGD step
    theta, theta_ok = guarded((D,))
    theta.copy_(torch.as_tensor(d.theta[0].copy()))
    loss = torch.zeros(1, device="cuda")
    plan.sgd_step(theta, x, y, lr, loss, batch=batch, row_idx=idx)
    torch.cuda.synchronize()
    theta_ok(f"{name} theta")
    assert abs(float(loss) - ref_loss) <= cc.TOL * abs(ref_loss)
    close_increment(theta.cpu().numpy(), d.theta[0], d.theta[0].astype(np.float64) - lr * ref_grad, spec, f"{name} SGD step")
    # three chained SWAG steps from the device's own state
    rng = np.random.default_rng(5)
    rms = float(np.sqrt(np.mean(d.theta[0].astype(np.float64) ** 2)))
    state = {}
    for key, init in (("theta", d.theta[0]), ("mean", d.theta[0] + 0.1 * rms * rng.normal(size=D)),
                      ("sq", d.theta[0].astype(np.float64) ** 2 + (0.05 * rms) ** 2)):
        state[key], ok = guarded((D,))
        state[key].copy_(torch.as_tensor(np.array(init, dtype=np.float32)))
        state[key + "_ok"] = ok
    dev, dev_ok = guarded((2, D))
    dev.copy_(torch.as_tensor(rng.normal(size=(2, D)).astype(np.float32)))
    n0 = 3
    for k, (update, row) in enumerate(SWAG_STEPS):
        s0 = {key: state[key].cpu().numpy().copy() for key in ("theta", "mean", "sq")}
        dev0 = dev.cpu().numpy().copy()
        assert cc.margin_of(name, batch, s0["theta"]) > cc.MARGIN, f"{name} SWAG step {k}: the chained state sits on a tie"
        l64, g64, _, _ = cc.loss_grad(spec, s0["theta"].astype(np.float64), xb, yb)
        assert min(cc.block_scales(g64, spec).values()) > 0.0, f"{name} SWAG step {k}: a block's reference gradient is zero"
        plan.swag_step(state["theta"], state["mean"], state["sq"], dev[row] if row is not None else None, x, y, lr, n0 + k,
                       update, loss, batch=batch, row_idx=idx)
        torch.cuda.synchronize()
        for key in ("theta", "mean", "sq"):
            state[key + "_ok"](f"{name} SWAG step {k}: {key}")
        dev_ok(f"{name} SWAG step {k}: deviation rows")
        got = {key: state[key].cpu().numpy() for key in ("theta", "mean", "sq")}
        what = f"{name} SWAG step {k}"
        assert abs(float(loss) - l64) <= cc.TOL * abs(l64), (what, float(loss), l64)
        close_increment(got["theta"], s0["theta"], s0["theta"].astype(np.float64) - lr * g64, spec, what)
        if update:
            th1 = got["theta"].astype(np.float64)
            _moment(got["mean"], s0["mean"], th1, float(n0 + k), f"{what}: mean")
            _moment(got["sq"], s0["sq"], th1 * th1, float(n0 + k), f"{what}: sq_mean")
        else:
            _same_bits(got["mean"], s0["mean"], f"{what}: mean on a step without update")
            _same_bits(got["sq"], s0["sq"], f"{what}: sq_mean on a step without update")
        dev1 = dev.cpu().numpy()
        for r in range(2):
            if update and r == row:
                _same_bits(dev1[r], got["theta"] - got["mean"], f"{what}: deviation row {r} is theta - mean")
            else:
                _same_bits(dev1[r], dev0[r], f"{what}: deviation row {r}, which this step does not write")
    plan.check_finite()


# ---------------------------------------------------------------- read-out
@pytest.mark.parametrize("name", cc.ALL)
def test_predict_five_draws_on_37_rows(gpu_device, name):
    from bayesian_inference_for_nn_amd.engine import ConvPlan
    case = cc.CASES[name]
    d = cc.make(name, case.batches[-1])
    spec = case.spec()
    rng = np.random.default_rng(11)
    S, n = 5, 37
    x = rng.normal(size=(n, int(np.prod(case.shape)))).astype(np.float32)
    W = (d.theta[0][None] * (1.0 + 0.05 * rng.normal(size=(S, spec.n_params)))).astype(np.float32)
    W[3, -1] = np.nan                       # the last bias of draw 3: one output column of that draw is NaN -> counts as 0
    ref = np.stack([cc.forward(spec, W[s].astype(np.float64), x.astype(np.float64))["out"] for s in range(S)])
    ref = np.nan_to_num(ref, nan=0.0)
    plan = ConvPlan(spec, max_batch=n, max_particles=2)         # the draws go through in chunks of 2, 2, 1
    samples, mean = plan.predict(torch.as_tensor(W).cuda(), torch.as_tensor(x).cuda())
    torch.cuda.synchronize()
    assert not torch.isnan(samples).any() and not torch.isnan(mean).any()
    e = {f"draw {s}": cc.rel(samples[s].cpu().numpy(), ref[s]) for s in range(S)}
    e["mean"] = cc.rel(mean.cpu().numpy(), ref.mean(axis=0))
    cc.assert_close(e, f"{name}: predict")
    mean2, m2 = plan.predict_moments(torch.as_tensor(W).cuda(), torch.as_tensor(x).cuda())
    e = {"mean": cc.rel(mean2.cpu().numpy(), ref.mean(axis=0)),
         "m2": cc.rel(m2.cpu().numpy(), np.einsum("snc,snd->ncd", ref, ref))}
    cc.assert_close(e, f"{name}: predict_moments")
    _, mean_only = plan.predict(torch.as_tensor(W).cuda(), torch.as_tensor(x).cuda(), want_samples=False)
    assert np.array_equal(bits(mean_only), bits(mean))
    with pytest.raises(ValueError):
        plan.predict(torch.as_tensor(W).cuda(), torch.as_tensor(np.zeros((n + 1, x.shape[1]), dtype=np.float32)).cuda())


def test_a_dense_model_launches_none_of_the_new_kernels(gpu_device):
    from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPPlan, MLPSpec
    spec = MLPSpec((20, 16, 4), ("relu", "softmax"), "scce")
    plan = MLPPlan(spec, max_batch=33)
    rng = np.random.default_rng(0)
    th = torch.as_tensor((0.3 * rng.normal(size=spec.n_params)).astype(np.float32)).cuda()
    x = torch.as_tensor(rng.normal(size=(33, 20)).astype(np.float32)).cuda()
    y = torch.as_tensor(rng.integers(0, 4, size=33).astype(np.int32)).cuda()
    with KernelProbe() as kp:
        plan.forward(th, x)
        plan.loss_grad(th, x, y)
        plan.sgd_step(th.clone(), x, y, 0.1, torch.zeros(1, device="cuda"))
        plan.predict(th[None].contiguous(), x)
    names = [n for n, _ in kp.launches]
    assert names and not [n for n in names if any(k in n for k in NEW_KERNELS)], names


def test_batch_outside_the_plan_is_refused(gpu_device):
    from bayesian_inference_for_nn_amd import _lib
    from bayesian_inference_for_nn_amd._lib import ptr
    d = cc.make("E", 5)
    plan = plan_of(d.case, 5, slack=0)
    theta = torch.as_tensor(d.theta[0].copy()).cuda()
    x = upload_x(d.x)
    with pytest.raises(ValueError, match="batch"):
        plan.forward(theta, x, batch=6)
    out = torch.zeros(9 * plan.F, device="cuda")
    rc = plan.lib.pyz_stem_forward(plan.h, ptr(theta), plan.D, 1, ptr(x), None, 6, ptr(out), None)
    assert rc == -2 and b"batch 6 outside" in plan.lib.pyz_last_error()
    rc = plan.lib.pyz_stem_forward(plan.h, ptr(theta), plan.D, 2, ptr(x), None, 5, ptr(out), None)
    assert rc == -2
    with pytest.raises(_lib.PyzError):
        _lib.check(rc)


def test_a_binary_crossentropy_plan_is_refused_by_every_conv_entry_point(gpu_device):
    """The conv net's loss kernels have no BinaryCrossentropy arm: a Dense plan with that loss is refused, not run as MSE."""
    from bayesian_inference_for_nn_amd._lib import ptr
    from bayesian_inference_for_nn_amd.engine import MLPPlan, MLPSpec
    d = cc.make("E", 5)
    plan = plan_of(d.case, 5, slack=0)
    bce = MLPPlan(MLPSpec((plan.F, 1), ("sigmoid",), "bce"), max_batch=5)
    theta = torch.zeros(plan.D_stem + bce.D, device="cuda")
    x, out = upload_x(d.x), torch.zeros(64, device="cuda")
    y = torch.zeros((len(d.x), 1), device="cuda")
    lib = plan.lib
    calls = (lambda: lib.pyz_convnet_forward(plan.h, bce.h, ptr(theta), 1, ptr(x), None, 5, ptr(out), None),
             lambda: lib.pyz_convnet_loss_grad(plan.h, bce.h, ptr(theta), 1, ptr(x), ptr(y), None, 5, None, ptr(out), None),
             lambda: lib.pyz_convnet_sgd_step(plan.h, bce.h, ptr(theta), ptr(x), ptr(y), None, 5, 0.1, ptr(out), None),
             lambda: lib.pyz_convnet_swag_step(plan.h, bce.h, ptr(theta), ptr(theta), ptr(theta), None, ptr(x), ptr(y), None, 5,
                                               0.1, 0, 1, ptr(out), None),
             lambda: lib.pyz_convnet_predict(plan.h, bce.h, ptr(theta), 1, ptr(x), 5, None, ptr(out), None, None))
    for call in calls:
        assert call() == -1 and b"BinaryCrossentropy" in lib.pyz_last_error()
    torch.cuda.synchronize()
    assert not theta.any()


# ---------------------------------------------------------------- end to end: SWAG, result(), store / load
def toy_dataset():
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
    x, y = cc.toy_data()
    return Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=0)


def toy_swag(seed=3):
    from bayesian_inference_for_nn_amd.nn.model import model_from_json
    from bayesian_inference_for_nn_amd.optimizers import SWAG
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    hp = cc.TOY_HP
    cfg = cc.TOY.json()
    start = model_from_json(cfg)
    start.reset_glorot(np.random.default_rng(seed))
    opt = SWAG()
    opt.compile(HyperParameters(lr=hp["lr"], k=hp["k"], frequency=hp["frequency"], scale=hp["scale"], batch_size=hp["batch_size"]),
                cfg, toy_dataset(), verbose=False, seed=seed, starting_model=start)
    return opt


def recorded(opt):
    """opt.step, recording the loss of every call."""
    losses, inner = [], opt.step

    def step(path=None):
        loss = inner(path)
        losses.append(loss)
        return loss
    opt.step = step
    return losses


@pytest.mark.parametrize("how", ["step", "quiet train"])
def test_swag_trains_the_toy_task(gpu_device, how, tmp_path):
    from bayesian_inference_for_nn_amd.distributions import tfd
    from bayesian_inference_for_nn_amd.engine import ConvPlan
    from bayesian_inference_for_nn_amd.nn import BayesianModel
    opt = toy_swag()
    assert isinstance(opt._plan, ConvPlan) and not opt._resident_supported()
    steps = cc.TOY_HP["steps"]
    if how == "step":
        losses = [opt.step() for _ in range(steps)]
    else:
        losses = recorded(opt)
        opt.train(steps)                    # quiet: must fall back to the step loop
        assert len(losses) == steps
    losses = [float(l) for l in losses]
    first, last = float(np.mean(losses[:20])), float(np.mean(losses[-20:]))
    print(f"toy task through {how}: first 20 {first:.4f}, last 20 {last:.4f}")
    assert np.isfinite(losses).all() and last < 0.5 * first
    if how != "step":
        return
    # the read-outs of result()
    bm = opt.result()
    x, y = cc.toy_data(seed=1)
    tfd.seed(7)
    samples, mean = bm.predict(x[:50], 6)
    assert len(samples) == 6 and mean.shape == (50, 2)
    assert (np.argmax(mean, axis=1) == y[:50]).mean() > 0.9
    tfd.seed(7)
    m, m2, n = bm.predictive_moments(x[:50], 6)
    assert n == 6 and np.abs(m - np.asarray(mean)).max() <= 1e-6
    assert np.abs(m2 - np.einsum("snc,snd->ncd", np.stack(samples), np.stack(samples))).max() <= 1e-5
    assert bm.predictive_mean(x[:50], 4).shape == (50, 2)
    assert bm.sample_model().predict(x[:5]).shape == (5, 2)
    score = bm.corruption_scores(x[:50] * 255.0, y[:50], (8, 8, 1), 0, severities=(1,), nb_samples=4)
    assert score.shape == (1,) and 0.0 <= score[0] <= 1.0
    # store / load: the Keras JSON, and equal draws under the same seed
    bm.store(str(tmp_path / "m"))
    assert json.load(open(os.path.join(str(tmp_path / "m"), "config.json"))) == json.loads(cc.TOY.json())
    loaded = BayesianModel.load(str(tmp_path / "m"))
    tfd.seed(9)
    a = bm.predict(x[:20], 5)[1]
    tfd.seed(9)
    b = loaded.predict(x[:20], 5)[1]
    assert np.array_equal(np.asarray(a), np.asarray(b))


def test_sgd_trains_and_metrics_read_the_result(gpu_device):
    from bayesian_inference_for_nn_amd.nn.model import model_from_json
    from bayesian_inference_for_nn_amd.optimizers import SGD
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    from bayesian_inference_for_nn_amd.visualisations import Metrics
    cfg, ds = cc.TOY.json(), toy_dataset()
    start = model_from_json(cfg)
    start.reset_glorot(np.random.default_rng(2))
    opt = SGD()
    opt.compile(HyperParameters(lr=0.05, frequency=1, batch_size=32), cfg, ds, verbose=False, seed=2, starting_model=start)
    assert not opt._resident_supported()
    opt.train(60)
    acc = Metrics(opt.result(), ds).accuracy(n_samples=3)
    assert acc > 0.9, acc


def test_image_script_recipe_runs_through_compat(gpu_device, monkeypatch):
    """The recipe of the reference's image script (tests/tf_dataset_test.py:42-84: a Keras Sequential of Conv2D(same, relu),
    Flatten, Dense(relu), Dense(softmax) built with the TensorFlow stand-in, SWAG from that model as starting_model,
    Metrics on the result), at 8 x 8 x 3 with 8 filters and 16 hidden units."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "compat"))
    sys.modules.pop("tensorflow", None)
    import tensorflow as tf
    try:
        from bayesian_inference_for_nn_amd.datasets import Dataset
        from bayesian_inference_for_nn_amd.optimizers import SWAG
        from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
        from bayesian_inference_for_nn_amd.visualisations import Metrics
        L = tf.keras.layers
        rng = np.random.default_rng(0)
        y = rng.integers(0, 10, size=200).astype(np.int32)
        x = (rng.normal(size=(200, 8, 8, 3)) * 0.1 + (y[:, None, None, None] / 10.0)).astype(np.float32)
        data = Dataset((x, y), tf.keras.losses.SparseCategoricalCrossentropy, "Classification", seed=0)
        net = tf.keras.Sequential()
        for layer in (L.Conv2D(8, 3, padding="same", activation="relu", input_shape=(8, 8, 3)), L.Flatten(),
                      L.Dense(16, activation="relu"), L.Dense(10, activation="softmax")):
            net.add(layer)
        swag = SWAG()
        swag.compile(HyperParameters(lr=1e-3, k=5, frequency=1, scale=1, batch_size=128), net.to_json(), data,
                     starting_model=net, verbose=False)
        swag.train(8)
        out = Metrics(swag.result(), data).summary(10, n_samples=3)
        assert set(out) >= {"accuracy", "ece"} and np.isfinite(out["accuracy"])
    finally:
        sys.modules.pop("tensorflow", None)


# ---------------------------------------------------------------- refusals of the Python surface
@pytest.mark.parametrize("which", ["ADAM", "VADAM", "BSAM", "SGLD", "BBB", "HMC", "SVGD", "FSVI"])
def test_other_optimizers_refuse_a_conv_model(gpu_device, which):
    from bayesian_inference_for_nn_amd import optimizers
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    hp = dict(lr=0.01, batch_size=32, frequency=1, k=3, scale=1.0, alpha=0.0, pi=0.5, beta_1=0.9, beta_2=0.999, lam=1.0, rho=0.05,
              gam=0.1, epsilon=0.01, m=1, L=2, M=2, gamma=0.1, num_data=256)
    opt = getattr(optimizers, which)()
    with pytest.raises(ValueError) as e:
        opt.compile(HyperParameters(**hp), cc.TOY.json(), toy_dataset(), verbose=False, seed=0,
                    starting_model=None, prior=None, n_chains=1)
    assert which in str(e.value) and "SGD and SWAG" in str(e.value), str(e.value)


@pytest.mark.parametrize("which", ["SGD", "SWAG"])
def test_members_refuse_a_conv_model(gpu_device, which):
    from bayesian_inference_for_nn_amd import optimizers
    from bayesian_inference_for_nn_amd.nn.model import model_from_json
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    opt = getattr(optimizers, which)()
    with pytest.raises(ValueError) as e:
        opt.compile(HyperParameters(lr=0.01, batch_size=32, frequency=1, k=3, scale=1.0), cc.TOY.json(), toy_dataset(),
                    verbose=False, seed=0, starting_model=model_from_json(cc.TOY.json()), n_members=2)
    assert which in str(e.value) and "n_members" in str(e.value) and "SGD and SWAG" in str(e.value)


def test_read_outs_without_a_conv_form_refuse(gpu_device):
    bm = toy_swag().result()
    x, y = cc.toy_data()
    for call in (lambda: bm.adversarial_examples(x[:4], y[:4], "scce", 0.1, 2), lambda: bm.predictive_surface(x[:4], 2),
                 lambda: bm.grid_surface(np.zeros((64, 2)), 0, 1, 2, 0, 1, 2, 2)):
        with pytest.raises(ValueError, match="conv model"):
            call()
