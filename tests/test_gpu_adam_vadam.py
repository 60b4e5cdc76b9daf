"""ADAM / VADAM on the device against the restatement of tests/adam_checks.py (per-example gradients from the oracle,
one row at a time): the fused step (last layer <= 32 units: gradients, squared-gradient means and update in
k_wgrad_adam) and the unfused one (k_dense_bwd_weight_sq + k_adam_update), every workgroup size the weight-gradient
launch picks (S = 1 / 2 / 4 / 8 / 16 waves), ragged last batches, epoch changes inside a run, the VADAM perturbation
(injected and Philox noise), and the optimizer classes.  Tolerances as tests/test_gpu_parity.py: float32 kernels
against float64, 1e-4 relative to the largest reference magnitude."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from adam_checks import AdamRef, epoch_plan, grad_moments
from oracle import mlp as o_mlp
from oracle import philox as o_philox

from bayesian_inference_for_nn_amd import synth
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.distributions import tfd
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
from bayesian_inference_for_nn_amd.nn import BayesianModel, model_from_json, sequential_json
from bayesian_inference_for_nn_amd.optimizers import ADAM, VADAM
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters


def close(gpu, ref, rel=1e-4, what=""):
    gpu = np.asarray(gpu.detach().cpu().numpy() if hasattr(gpu, "detach") else gpu, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(gpu - ref).max()
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e})"


@pytest.fixture(scope="module")
def eng(gpu_device):
    from bayesian_inference_for_nn_amd import engine
    return engine


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def make(spec, n, seed=0, scale=0.3):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, spec.dims[0])).astype(np.float32)
    if spec.loss == "scce":
        y = rng.integers(0, spec.dims[-1], size=n).astype(np.int32)
    else:
        y = rng.normal(size=(n, spec.dims[-1])).astype(np.float32)
    theta = (rng.normal(size=spec.n_params) * scale).astype(np.float32)
    return x, y, theta


def ydev(spec, y):
    return dev(y, torch.int32 if spec.loss == "scce" else torch.float32)


# name -> (spec, rows, batch).  Batches are chosen so that the launches pick every workgroup size of the weight-gradient
# kernels (S = waves per workgroup, pyz_pick_waves: steps = (batch + 1) / 2; S = 1 below 16 steps, 2 below 32, 4 below
# 64, 8 below 128, else 16), with odd ragged last batches (the peeled odd row) and several epochs per run.
MODELS = {
    "scce_s4_s1": (o_mlp.MLPSpec((20, 16, 4), ("relu", "softmax"), "scce"), 151, 64),            # 64, 64, 23
    "mse_s8_s2": (o_mlp.MLPSpec((6, 12, 8, 3), ("tanh", "sigmoid", "linear"), "mse"), 301, 128),  # 128, 128, 45
    "scce_s16_s4": (o_mlp.MLPSpec((30, 24, 5), ("tanh", "softmax"), "scce"), 601, 256),           # 256, 256, 89
    "one_layer_gathered": (o_mlp.MLPSpec((7, 3), ("softmax",), "scce"), 50, 21),                  # layer 0 gathers rows
    # last layer wider than 32 units: the unfused path
    "unfused_scce": (o_mlp.MLPSpec((12, 20, 40), ("tanh", "softmax"), "scce"), 91, 40),
    "unfused_mse": (o_mlp.MLPSpec((9, 16, 48), ("relu", "linear"), "mse"), 70, 33),
}


def run_pair(eng, name, steps, lr, beta_1, beta_2, vadam_lam=None, seed=0):
    """`steps` device steps and restated steps on the same batches; returns (plan tensors, restatement, losses)."""
    spec, n, batch = MODELS[name]
    x, y, theta0 = make(spec, n, seed=sum(map(ord, name)) + seed)
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=batch)
    th, m, v = dev(theta0), torch.zeros(spec.n_params, device="cuda"), torch.zeros(spec.n_params, device="cuda")
    loss = torch.zeros(1, device="cuda")
    xd, yd = dev(x), ydev(spec, y)
    ref = AdamRef(theta0)
    rng = np.random.default_rng(7)
    got, want, epochs = [], [], []
    for s, (idx, epoch) in enumerate(epoch_plan(n, batch, steps, seed=3)):
        extra = {}
        if vadam_lam is not None:
            eps = rng.normal(size=spec.n_params).astype(np.float32)
            plan.vadam_perturb(th, v, vadam_lam, float(n), s, 99, eps=dev(eps))
            ref.perturb(eps.astype(np.float64), vadam_lam, float(n))
            lam_n = vadam_lam / float(n)
            extra = dict(denom_eps=lam_n, decay=lam_n)
        plan.adam_step(th, m, v, xd, yd, lr, beta_1, beta_2, epoch, loss, batch=len(idx), row_idx=dev(idx, torch.int32),
                       **extra)
        got.append(float(loss.item()))
        want.append(ref.step(x[idx], y[idx], spec, lr, beta_1, beta_2, epoch, **extra))
        epochs.append(epoch)
    plan.check_finite()
    assert len(set(epochs)) >= 3, "the run must cross epochs"
    return (th, m, v), ref, got, want


def check_pair(tensors, ref, got, want):
    th, m, v = tensors
    close(got, want, what="loss")
    close(th, ref.theta, what="theta")
    close(m, ref.m, what="m")
    close(v, ref.v, what="v")


@pytest.mark.parametrize("name", list(MODELS))
def test_adam_step_matches_restatement(eng, name):
    check_pair(*run_pair(eng, name, 21, 0.01, 0.9, 0.999))


def test_adam_beta2_one_minus_2_pow_52(eng):
    """beta_2 = 1 - 2^-52 (the reference drivers' value) rounds to 1.0 in float32; 1 - beta_2 and 1 - beta_2^epoch must
    come from float64 on the host, or v / v^ would be 0 / 0."""
    for name in ("scce_s4_s1", "unfused_scce"):
        tensors, ref, got, want = run_pair(eng, name, 20, 0.01, 0.9, 1.0 - 2.0 ** -52)
        check_pair(tensors, ref, got, want)
        assert torch.isfinite(tensors[0]).all() and float(tensors[2].abs().max()) > 0


@pytest.mark.parametrize("name", ["scce_s4_s1", "mse_s8_s2", "unfused_mse"])
def test_vadam_injected_noise_matches_restatement(eng, name):
    check_pair(*run_pair(eng, name, 20, 0.01, 0.9, 0.999, vadam_lam=0.5))


@pytest.mark.parametrize("dims,acts,loss,n,batch", [
    ((20, 16, 4), ("relu", "softmax"), "scce", 93, 93),
    ((9, 16, 48), ("relu", "linear"), "mse", 57, 57),
    ((784, 200, 10), ("relu", "softmax"), "scce", 1024, 1024),     # C2 shape (S = 16)
])
def test_beta2_zero_gives_the_squared_gradient_mean(eng, dims, acts, loss, n, batch):
    """beta_2 = 0: v after one step is the raw batch mean of the squared per-example gradients."""
    spec = o_mlp.MLPSpec(dims, acts, loss)
    if dims[0] == 784:
        x, y = synth.mnist_like(n, seed=5)
        theta = synth.glorot_uniform(dims, seed=6)
    else:
        x, y, theta = make(spec, n, seed=4)
    plan = eng.MLPPlan(eng.MLPSpec(dims, acts, loss), max_batch=batch)
    th, m, v = dev(theta), torch.zeros(spec.n_params, device="cuda"), torch.zeros(spec.n_params, device="cuda")
    lo = torch.zeros(1, device="cuda")
    idx = np.random.default_rng(1).permutation(n)[:batch].astype(np.int32)
    plan.adam_step(th, m, v, dev(x), ydev(spec, y), 0.001, 0.9, 0.0, 1, lo, batch=batch, row_idx=dev(idx, torch.int32))
    rl, g, s = grad_moments(theta, x[idx], y[idx], spec)
    close(v, s, what="v = mean squared per-example gradient")
    close(m, 0.1 * g, rel=2e-4, what="m = (1 - beta_1) g")
    close([lo.item()], [rl], what="loss")


def test_vadam_philox_perturbation(eng):
    """The device noise is Philox (seed, stream 5, step): two runs bit-identical, the oracle's stream, and the
    perturbation's spread is 1 / sqrt(N (v + lam))."""
    dims = (784, 200, 10)
    plan = eng.MLPPlan(eng.MLPSpec(dims, ("relu", "softmax"), "scce"), max_batch=8)
    D = plan.D
    v = torch.full((D,), 0.3, device="cuda")
    outs = []
    for _ in range(2):
        th = torch.zeros(D, device="cuda")
        plan.vadam_perturb(th, v, 0.5, 1000.0, 17, 12345)
        outs.append(th.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    sigma = 1.0 / np.sqrt(1000.0 * 0.8)
    ref = o_philox.normal(12345, 5, 17, D) * sigma
    np.testing.assert_allclose(outs[0], ref, rtol=0, atol=4e-6 * sigma * 8)
    assert abs(outs[0].mean()) < 5 * sigma / np.sqrt(D)
    assert abs(outs[0].std() / sigma - 1.0) < 0.01
    th2 = torch.zeros(D, device="cuda")
    plan.vadam_perturb(th2, v, 0.5, 1000.0, 18, 12345)                  # another step: other numbers
    assert not np.array_equal(th2.cpu().numpy(), outs[0])


# ------------------------------------------------------------------ the optimizer classes
MOONS_JSON = sequential_json(2, [16, 2], ["relu", "softmax"])


def _compiled(cls, seed=11, **hyp):
    x, y = synth.moons(500, seed=42)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
    start = model_from_json(MOONS_JSON)
    start.reset_glorot(np.random.default_rng(9))
    opt = cls()
    opt.compile(HyperParameters(**hyp), MOONS_JSON, ds, verbose=False, starting_model=start, seed=seed)
    return opt, start


@pytest.mark.parametrize("cls", [ADAM, VADAM])
def test_train_equals_steps_and_result(cls):
    hyp = dict(lr=0.01, beta_1=0.9, beta_2=0.999, batch_size=64)
    a, start = _compiled(cls, **hyp)
    np.testing.assert_array_equal(a._theta.cpu().numpy(), start.weights_flat)   # starting weights copied
    b, _ = _compiled(cls, **hyp)
    n_it = 30                                         # 400 training rows, batch 64: 7 batches per epoch
    a.train(n_it)
    first = None
    for _ in range(n_it):
        last = b.step()
        first = float(last) if first is None else first
    assert a._n == b._n == n_it and a._epoch_num == b._epoch_num == 5 and a._seen_batches == b._seen_batches
    for t in ("_theta", "_m_dev", "_v_dev", "_running_dev"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    assert np.isfinite(float(last)) and float(last) < first
    bm = a.result()
    assert isinstance(bm, BayesianModel)
    theta, v = a._theta.cpu().numpy(), a._v_dev.cpu().numpy()
    by_layer = {start: d._tf_distribution for (start, _), d in zip(bm._layers_dtbn_intervals, bm._distributions)}
    assert sorted(by_layer) == a._weight_layers_indices
    for sl, layer_idx in zip(a._spec.layer_slices(), a._weight_layers_indices):
        d = by_layer[layer_idx]
        np.testing.assert_array_equal(d.loc, theta[sl])                 # the final weights
        if cls is ADAM:
            assert isinstance(d, tfd.Deterministic)
        else:
            assert isinstance(d, tfd.Normal)
            np.testing.assert_array_equal(d.scale, v[sl])               # the raw second moment, as the reference


def test_vadam_lam_and_training_split_size():
    """`lam` from the hyper-parameters when given; N = the size of the training split (not the `num_data` the
    reference's drivers pass, which the reference ignores)."""
    opt, _ = _compiled(VADAM, lr=0.01, beta_1=0.9, beta_2=0.999, batch_size=64, lam=2.0, num_data=7)
    assert opt._lam == 2.0 and opt._num_data == float(opt._dataset.train_size) == 400.0
    dflt, _ = _compiled(VADAM, lr=0.01, beta_1=0.9, beta_2=0.999, batch_size=64)
    assert dflt._lam == 0.5
    for _ in range(3):
        assert np.isfinite(float(opt.step()))
