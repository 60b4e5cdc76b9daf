"""BSAM on the device against the restatement of tests/bsam_checks.py (float64, gradients from the oracle): the fused
step (last layer <= 32 units: ascent and update in the epilogues of k_wgrad_bsam<S, 0 / 1>) and the unfused one
(k_bsam_ascent / k_bsam_update), every workgroup size the weight-gradient launch picks (S = 1 / 2 / 4 / 8 / 16 waves),
gathered rows, odd ragged last batches, epoch changes inside a run, injected and Philox noise, the C2 shape, and the
optimizer class.  Tolerance as tests/test_gpu_parity.py: float32 kernels against float64, 1e-4 relative to the largest
reference magnitude (tests/test_bsam_host.py checks that float32 rounding alone stays below 1e-5 on these runs)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from bsam_checks import SETTINGS, BsamRef, make, models, run_ref
from oracle import mlp as o_mlp
from oracle import philox as o_philox

from bayesian_inference_for_nn_amd import _lib, synth
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.distributions import tfd
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
from bayesian_inference_for_nn_amd.nn import BayesianModel, model_from_json, sequential_json
from bayesian_inference_for_nn_amd.optimizers import BSAM
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

MODEL_NAMES = ["scce_s4_s1", "mse_s8_s2", "scce_s16_s4", "one_layer_gathered", "unfused_scce", "unfused_mse"]


def close(gpu, ref, rel=1e-4, what=""):
    gpu = np.asarray(gpu.detach().cpu().numpy() if hasattr(gpu, "detach") else gpu, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(gpu - ref).max()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e})"


@pytest.fixture(scope="module")
def eng(gpu_device):
    from bayesian_inference_for_nn_amd import engine
    return engine


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def ydev(spec, y):
    return dev(y, torch.int32 if spec.loss == "scce" else torch.float32)


def fresh_state(D, theta0):
    """theta, m = 0, v = 1 (BSAM.py:121-141) and the two-loss buffer."""
    return dev(theta0), torch.zeros(D, device="cuda"), torch.ones(D, device="cuda"), torch.zeros(2, device="cuda")


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_bsam_step_matches_restatement(eng, name, setting):
    """21 steps over at least three epochs, injected eps: theta, m, v and both losses of every step."""
    assert sorted(MODEL_NAMES) == sorted(models())
    spec, n, batch = models()[name]
    x, y, theta0 = make(spec, n, seed=sum(map(ord, name)))
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=batch)
    th, m, v, loss = fresh_state(spec.n_params, theta0)
    xd, yd = dev(x), ydev(spec, y)
    got = []

    def device_step(i, idx, eps):
        plan.bsam_step(th, m, v, xd, yd, num_data=float(n), step=i, seed=99, loss_out=loss, eps=dev(eps), batch=len(idx),
                       row_idx=dev(idx, torch.int32), **SETTINGS[setting])
        got.append(loss.cpu().numpy().astype(np.float64))

    ref, want = run_ref(name, setting, steps=21, on_step=device_step)
    plan.check_finite()
    close(np.asarray(got), np.asarray(want), what=f"{name}/{setting} losses (l1, l2)")
    close(th, ref.theta, what=f"{name}/{setting} theta")
    close(m, ref.m, what=f"{name}/{setting} m")
    close(v, ref.v, what=f"{name}/{setting} v")


@pytest.mark.parametrize("name", ["scce_s4_s1", "scce_s16_s4", "unfused_mse"])
def test_first_pass_state_with_zero_learning_rate(eng, name):
    """lr = 0: the update leaves the weights alone, so after one step theta = theta0 + eps / (N v0) + rho g1 / v0 with g1
    taken at the perturbed weights -- the first pass's epilogue on its own; m and v still move."""
    spec, n, batch = models()[name]
    x, y, theta0 = make(spec, n, seed=21)
    rng = np.random.default_rng(5)
    eps = rng.normal(size=spec.n_params).astype(np.float32)
    v0 = rng.uniform(0.5, 2.0, size=spec.n_params).astype(np.float32)
    idx = rng.permutation(n)[:batch].astype(np.int32)
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=batch)
    th, m, _, loss = fresh_state(spec.n_params, theta0)
    v = dev(v0)
    hyp = dict(SETTINGS["sharp"], lr=0.0, rho=0.05)
    plan.bsam_step(th, m, v, dev(x), ydev(spec, y), num_data=float(n), step=0, seed=1, loss_out=loss, eps=dev(eps),
                   batch=batch, row_idx=dev(idx, torch.int32), **hyp)
    pert = theta0.astype(np.float64) + eps.astype(np.float64) * (np.float64(np.float32(1.0 / n)) / v0)
    l1, g1 = o_mlp.loss_and_grad(pert, x[idx], y[idx], spec)[:2]
    asc = pert + np.float64(np.float32(0.05)) * g1 / v0
    close(th, asc, what="theta = perturbed + ascent")
    assert np.abs(asc - pert).max() > 1e-3 * np.abs(asc).max(), "the ascent must be visible at 1e-4"
    ref = BsamRef(theta0)
    ref.v = v0.astype(np.float64)
    want = ref.step(x[idx], y[idx], spec, eps, num_data=float(n), **hyp)
    close(loss, want, what="l1, l2")
    close([float(loss[0])], [l1], what="l1")
    close(m, ref.m, what="m")
    close(v, ref.v, what="v")


@pytest.mark.parametrize("name", ["scce_s4_s1", "unfused_scce"])
def test_philox_noise_is_the_oracle_stream(eng, name):
    """d_eps = NULL: the step equals the injected-noise step fed with the oracle's Philox normals of (seed, stream 6,
    step); another step value perturbs differently."""
    assert _lib.STREAM_BSAM == 6
    spec, n, batch = models()[name]
    x, y, theta0 = make(spec, n, seed=8)
    D = spec.n_params
    idx = dev(np.random.default_rng(2).permutation(n)[:batch].astype(np.int32), torch.int32)
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=batch)
    xd, yd = dev(x), ydev(spec, y)
    # N = 30: the perturbation (up to ~4 / 30) is a visible part of theta, and the device's float32 Box-Muller, which
    # differs from the oracle's float64 one by at most 3.2e-5 per normal (tests/test_gpu_adam_vadam.py), moves theta by at
    # most 1.1e-6 -- a hundredth of the standing tolerance
    hyp = dict(SETTINGS["sharp"], num_data=30.0)

    def one(step, eps=None):
        th, m, v, loss = fresh_state(D, theta0)
        plan.bsam_step(th, m, v, xd, yd, step=step, seed=12345, loss_out=loss, eps=eps, batch=batch, row_idx=idx, **hyp)
        return [t.cpu().numpy().astype(np.float64) for t in (th, m, v, loss)]

    own = one(17)
    injected = one(17, dev(o_philox.normal(12345, 6, 17, D).astype(np.float32)))
    for a, b, what in zip(own, injected, ("theta", "m", "v", "loss")):
        close(a, b, what=f"Philox against injected oracle normals: {what}")
    again = one(17)
    assert all(np.array_equal(a, b) for a, b in zip(own[:3], again[:3])), "same (seed, step): same step"
    other = one(18)
    assert np.abs(other[0] - own[0]).max() > 1e-2 * np.abs(own[0]).max(), "another step: another perturbation"
    wrong = one(17, dev(o_philox.normal(12345, 5, 17, D).astype(np.float32)))   # VADAM's stream is not BSAM's
    assert np.abs(wrong[0] - own[0]).max() > 1e-2 * np.abs(own[0]).max()


def test_c2_shape_one_step(eng):
    """784 -> 200 -> 10, batch 1024 (S = 16 waves per workgroup) against the restatement."""
    dims, acts = (784, 200, 10), ("relu", "softmax")
    spec = o_mlp.MLPSpec(dims, acts, "scce")
    n = batch = 1024
    x, y = synth.mnist_like(n, seed=5)
    theta0 = synth.glorot_uniform(dims, seed=6)
    eps = np.random.default_rng(3).normal(size=spec.n_params).astype(np.float32)
    idx = np.random.default_rng(1).permutation(n).astype(np.int32)
    plan = eng.MLPPlan(eng.MLPSpec(dims, acts, "scce"), max_batch=batch)
    th, m, v, loss = fresh_state(spec.n_params, theta0)
    plan.bsam_step(th, m, v, dev(x), ydev(spec, y), num_data=float(n), step=0, seed=1, loss_out=loss, eps=dev(eps),
                   batch=batch, row_idx=dev(idx, torch.int32), **SETTINGS["sharp"])
    plan.check_finite()
    ref = BsamRef(theta0)
    want = ref.step(x[idx], np.asarray(y)[idx], spec, eps, num_data=float(n), **SETTINGS["sharp"])
    close(loss, want, what="C2 l1, l2")
    close(th, ref.theta, what="C2 theta")
    close(m, ref.m, what="C2 m")
    close(v, ref.v, what="C2 v")


def test_argument_errors_return_invalid_without_launching(eng):
    spec, n, batch = models()["scce_s4_s1"]
    x, y, theta0 = make(spec, n, seed=1)
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=batch)
    th, m, v, loss = fresh_state(spec.n_params, theta0)
    xd, yd = dev(x), ydev(spec, y)
    good = dict(SETTINGS["sharp"], num_data=float(n), step=0, seed=1)
    for bad in (dict(beta_1=1.0), dict(beta_1=-0.1), dict(beta_2=1.0), dict(beta_2=float("nan")), dict(num_data=0.0),
                dict(num_data=-5.0), dict(step=-1)):
        with pytest.raises(_lib.PyzError) as e:
            plan.bsam_step(th, m, v, xd, yd, loss_out=loss, batch=batch, **dict(good, **bad))
        assert e.value.code == -1, bad                                     # PYZ_E_INVALID
    torch.cuda.synchronize()
    np.testing.assert_array_equal(th.cpu().numpy(), theta0)                # nothing ran
    assert float(v.min()) == float(v.max()) == 1.0 and float(m.abs().max()) == 0.0


# ------------------------------------------------------------------ the optimizer class
MOONS_JSON = sequential_json(2, [16, 2], ["relu", "softmax"])
HYP = dict(lr=0.01, beta_1=0.9, beta_2=0.9, lam=0.5, rho=0.01, gam=0.1, batch_size=64)


def _compiled(seed=11, **hyp):
    x, y = synth.moons(500, seed=42)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
    start = model_from_json(MOONS_JSON)
    start.reset_glorot(np.random.default_rng(9))
    opt = BSAM()
    opt.compile(HyperParameters(**hyp), MOONS_JSON, ds, verbose=False, starting_model=start, seed=seed)
    return opt, start, ds


def test_class_train_result_predict(tmp_path):
    a, start, ds = _compiled(**HYP)
    np.testing.assert_array_equal(a._theta.cpu().numpy(), start.weights_flat)   # starting weights copied
    assert float(a._v_dev.min()) == float(a._v_dev.max()) == 1.0 and float(a._m_dev.abs().max()) == 0.0
    assert a._num_data == float(ds.train_size) == 400.0
    b, _, _ = _compiled(**HYP)
    n_it = 30                                         # 400 training rows, batch 64: 7 batches per epoch
    a.train(n_it)
    path = str(tmp_path / "losses.txt")
    pairs, last = [], None
    for _ in range(n_it):
        last = b.step(path)
        pairs.append(b._loss_dev.cpu().numpy().astype(np.float64))
    assert a._n == b._n == n_it and a._epoch_num == b._epoch_num == 5 and a._seen_batches == b._seen_batches == 2
    for t in ("_theta", "_m_dev", "_v_dev", "_running_dev"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    # the returned loss: (sum of l1 + l2 over the batches of the current epoch) / seen batches  (BSAM.py:73,97,119)
    want = sum(p.sum() for p in pairs[-b._seen_batches:]) / b._seen_batches
    assert abs(float(last) - want) <= 1e-6 * abs(want), (float(last), want)
    assert open(path).read() == "".join(str(float(np.float32(l))) for p in pairs for l in p)   # l1 then l2, every step
    a._plan.check_finite()
    assert np.isfinite(float(last))
    bm = a.result()
    assert isinstance(bm, BayesianModel)
    theta, v = a._theta.cpu().numpy(), a._v_dev.cpu().numpy()
    by_layer = {s: d._tf_distribution for (s, _), d in zip(bm._layers_dtbn_intervals, bm._distributions)}
    assert sorted(by_layer) == a._weight_layers_indices
    for sl, layer_idx in zip(a._spec.layer_slices(), a._weight_layers_indices):
        d = by_layer[layer_idx]
        assert isinstance(d, tfd.Normal)
        np.testing.assert_array_equal(d.loc, theta[sl])                                  # the final weights
        np.testing.assert_allclose(d.scale, 1.0 / (400.0 * v[sl].astype(np.float64)), rtol=1e-6)   # 1 / (N v)
    assert (v != 1.0).any() and (v > 0).all()
    x, _ = synth.moons(50, seed=1)
    samples, pred = bm.predict(x.astype(np.float32), 4)
    assert len(samples) == 4 and np.isfinite(np.asarray(pred)).all()
