"""CPU checks of FSVI: the restatement of tests/fsvi_checks.py against torch autograd on the reference's literal
expressions (Pyesian/optimizers/FSVI.py:95-136, 149-195), its sensitivity to the quirks it keeps, the exports, and the
argument errors of the C ABI that need no device."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fsvi_checks as fc
from bayesian_inference_for_nn_amd import _lib

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
F64 = torch.float64


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


# ---------------------------------------------------------------- the reference's expressions, in torch
def torch_model(theta, x, spec):
    """The Keras Dense stack on the flat float64 parameter tensor theta."""
    h, off = x, 0
    for i, o, a in zip(spec.dims[:-1], spec.dims[1:], spec.acts):
        w = theta[off:off + i * o].reshape(i, o)
        b = theta[off + i * o:off + (i + 1) * o]
        off += (i + 1) * o
        h = h @ w + b
        h = {"linear": lambda v: v, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[a](h)
    return h


def torch_gp_log_likelihood(f, x, jitter=1e-6):
    """_gp_log_likelihood (FSVI.py:149-165): ExponentiatedQuadratic(1, 1) + jitter, zero-mean MVN log_prob of f[:, 0]."""
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    K = torch.exp(-d2 / 2.0) + jitter * torch.eye(len(x), dtype=F64)
    mvn = torch.distributions.MultivariateNormal(torch.zeros(len(x), dtype=F64), covariance_matrix=K)
    return mvn.log_prob(f[:, 0])


def torch_stein_gradient(w, sigma=1.0, reg=1e-3):
    """_stein_gradient with _rbf_kernel and _grad_rbf_kernel, line by line (FSVI.py:177-195)."""
    n = w.shape[0]
    x = w.unsqueeze(-1)
    diff = x.unsqueeze(1) - x.unsqueeze(0)
    K = torch.exp(-(diff ** 2).sum(-1) / (2.0 * sigma ** 2))
    K_reg = K + reg * torch.eye(n, dtype=F64)
    grad_K = -diff / (sigma ** 2) * K.unsqueeze(-1)
    b = (1.0 / n) * grad_K.sum(dim=1)
    return -torch.linalg.solve(K_reg, b)


def problem(name, k, B, b, seed):
    spec = fc.specs()[name]
    x, y, mu, W = fc.make_problem(spec, rows=max(b, 4), B=B, k=k, seed=seed)
    rng = np.random.default_rng(seed + 1)
    xm = rng.uniform(-30, 30, size=(B, spec.dims[0])).astype(np.float32)
    z = (0.1 * rng.normal(size=(k, spec.dims[0]))).astype(np.float32)
    return spec, x[:b], y[:b], W, xm, z


# ---------------------------------------------------------------- the terms
@pytest.mark.parametrize("points", ["spread", "near"])
def test_gp_gradient_is_minus_alpha(points):
    """d gp_ll / d f = -K^-1 f, against autograd through MultivariateNormal.log_prob, to 1e-9."""
    rng = np.random.default_rng(3)
    if points == "spread":
        x = rng.uniform(-30, 30, size=(20, 2)).astype(np.float32)
    else:
        x = np.linspace(-4, 4, 9).astype(np.float32).reshape(-1, 1)        # neighbours one length scale apart
    f = rng.normal(size=len(x))
    ft = t64(f).reshape(-1, 1).requires_grad_(True)
    torch_gp_log_likelihood(ft, t64(x)).backward()
    want = ft.grad.numpy().reshape(-1)
    got = -fc.gp_alpha(fc.gram(x), f)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"{points}: rel {rel:.3e}, cond {np.linalg.cond(fc.gram(x)):.3e}")
    assert rel <= 1e-9


@pytest.mark.parametrize("D", [3, 33, 151])
def test_stein_term_equals_the_literal_expressions(D):
    w = (np.random.default_rng(D).normal(size=D)).astype(np.float32)
    want = torch_stein_gradient(t64(w)).numpy().reshape(-1)
    got = fc.stein_c2(w)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    A, rhs = fc.stein_system(w)
    assert np.array_equal(A, A.T) and A[0, 0] == 1.0 + 1e-3 and rhs.shape == (D,)


@pytest.mark.parametrize("name,k,b", [("dense1", 1, 5), ("dense1", 3, 5), ("tanh8", 3, 5), ("relu88", 3, 5), ("tanh8", 2, 1)])
def test_merged_delta_equals_the_three_tape_gradients(name, k, b):
    """g of the restatement (one backward pass per particle through the merged output delta) against the reference's
    three separate gradients -- dll (FSVI.py:95-98), c1 (:107-112), c2 (:114) combined as :115-136 -- by autograd."""
    B = 5
    spec, xd, y, W, xm, z = problem(name, k, B, b, seed=11)
    out = fc.terms(W, xd, y, xm, z, spec, B)
    xp = out["xp"]
    total_dll = torch.zeros(spec.n_params, dtype=F64)
    total_dkl = torch.zeros(spec.n_params, dtype=F64)
    loss = 0.0
    for i in range(k):
        th = t64(W[i]).requires_grad_(True)
        batch_X, full = t64(xp[i][:b]), t64(xp[i])
        ll = ((torch_model(th, batch_X, spec) - t64(y).reshape(b, 1)) ** 2).mean()       # loss()(y_pred_d, batch_Y)
        dll, = torch.autograd.grad(ll, th)
        total_dll += (1 / B * k) * dll                                                   # :98
        gp = torch_gp_log_likelihood(torch_model(th, full, spec), full)
        c1, = torch.autograd.grad(gp, th)
        c2 = torch_stein_gradient(t64(W[i])).reshape(-1).to(torch.float32).to(F64)       # :115 casts it to float32
        total_dkl += (1 / k) * (c2 - c1)                                                 # :115-116
        loss += float(ll.detach()) / k
    want = (total_dll - total_dkl).numpy()                                               # :136
    err = np.abs(out["g"] - want).max() / np.abs(want).max()
    print(f"{name} k={k} b={b}: rel err {err:.3e}")
    assert err <= 1e-10
    assert abs(out["loss"] - loss) <= 1e-12 * abs(loss)


def test_inputs_are_float32_and_keep_the_prefix_sum():
    spec, xd, y, W, xm, z = problem("dense1", 3, 4, 3, seed=2)
    xp = fc.make_xp(xd, xm, z)
    assert xp.dtype == np.float32 and xp.shape == (3, 7, 2)
    np.testing.assert_array_equal(xp[1][:3], xd + z[1])                         # the batch rows: a fresh z_i
    np.testing.assert_array_equal(xp[0][3:], xm + z[0])
    np.testing.assert_array_equal(xp[2][3:], xm + ((z[0] + z[1]) + z[2]))       # the measurement rows: the running sum
    fresh = fc.make_xp(xd, xm, z, shift="fresh")
    np.testing.assert_array_equal(fresh[0], xp[0])                              # only shows for k >= 2
    assert np.abs(fresh[2] - xp[2]).max() > 0.01


def test_wrong_variants_are_visible():
    """A fresh shift of the measurement rows, or k / B read as 1 / (B k), must move g by far more than any tolerance."""
    B, k = 5, 3
    spec, xd, y, W, xm, z = problem("tanh8", k, B, 5, seed=5)
    z = z * 10.0                                # noise on the kernel's length scale, so that the shift matters to K_i
    xm = xm / 10.0                              # ... and measurement points close enough to interact
    right = fc.terms(W, xd, y, xm, z, spec, B)["g"]
    scale = np.abs(right).max()
    fresh = fc.terms(W, xd, y, xm, z, spec, B, shift="fresh")["g"]
    assert np.abs(fresh - right).max() > 1e-2 * scale
    swapped = fc.terms(W, xd, y, xm, z, spec, B, data_scale=1.0 / (B * k))["g"]
    assert np.abs(swapped - right).max() > 1e-2 * scale
    one = fc.terms(W[:1], xd, y, xm, z[:1], spec, B)["g"]
    assert np.array_equal(one, fc.terms(W[:1], xd, y, xm, z[:1], spec, B, shift="fresh")["g"])


def test_adam_is_the_legacy_update():
    mu, g = np.array([1.0, -2.0]), np.array([0.5, -0.25])
    new, m, v = fc.adam(mu, g, np.zeros(2), np.zeros(2), 1, 0.1)
    np.testing.assert_allclose(new, mu - 0.1 * np.sign(g), rtol=1e-5)           # the first step is lr sign(g)
    np.testing.assert_allclose(m, 0.1 * g)
    np.testing.assert_allclose(v, 0.001 * g * g)


def test_philox_draws_use_stream_nine_and_the_step_indices():
    from oracle import philox
    assert _lib.STREAM_FSVI == fc.STREAM == 9
    lo, hi = np.array([-1.0, 2.0], np.float32), np.array([3.0, 2.5], np.float32)
    xm = fc.draw_xm(7, 5, 6, 2, lo, hi)
    assert xm.shape == (6, 2) and (xm >= lo).all() and (xm < hi).all()
    u = philox.uniform(7, 9, 20, 12).reshape(6, 2)
    np.testing.assert_allclose(xm, lo + u * (hi - lo), rtol=1e-6)
    np.testing.assert_allclose(fc.draw_noise(7, 5, 3, 2).reshape(-1), 0.1 * philox.normal(7, 9, 21, 6), rtol=1e-6)
    np.testing.assert_allclose(fc.draw_eps(7, 5, 3, 4).reshape(-1), philox.normal(7, 9, 22, 12), rtol=1e-6)


# ---------------------------------------------------------------- exports and the C ABI
def test_exported_from_the_package_and_from_compat():
    from bayesian_inference_for_nn_amd.optimizers import FSVI, Optimizer
    assert issubclass(FSVI, Optimizer)
    code = "from Pyesian.optimizers import FSVI; import bayesian_inference_for_nn_amd.optimizers as o; assert FSVI is o.FSVI"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_deviations_are_in_the_docstring():
    from bayesian_inference_for_nn_amd.optimizers import FSVI as mod
    doc = sys.modules[mod.__module__].__doc__
    for word in ("Deviations", "float64", "Philox", "step 250", "sentinel"):
        assert word in doc, word


def _check(dims, acts, loss, k=2, batch=4, batch_size=4):
    lib = _lib.load()
    rc = lib.pyz_fsvi_check(len(acts), (C.c_int32 * len(dims))(*dims), (C.c_int32 * len(acts))(*[_lib.ACT[a] for a in acts]),
                            _lib.LOSS[loss], k, batch, batch_size)
    return rc, lib.pyz_last_error().decode()


def test_argument_errors_need_no_gpu():
    assert _check((2, 8, 1), ("tanh", "linear"), "mse")[0] == 0
    for kw, word in ((dict(dims=(2, 8, 3), acts=("relu", "softmax"), loss="scce"), "MeanSquaredError"),
                     (dict(dims=(2, 8, 1), acts=("relu", "softmax"), loss="mse"), "softmax"),
                     (dict(dims=(2, 8, 2), acts=("relu", "linear"), loss="mse"), "one unit"),
                     (dict(dims=(2, 8, 1), acts=("relu", "sigmoid"), loss="bce"), "MeanSquaredError"),
                     (dict(dims=(2, 1), acts=("linear",), loss="mse", k=0), "k >= 1"),
                     (dict(dims=(2, 1), acts=("linear",), loss="mse", batch=5, batch_size=4), "batch"),
                     (dict(dims=(2, 1), acts=("linear",), loss="mse", batch=512, batch_size=513), "1024"),
                     (dict(dims=(2, 1000, 1), acts=("relu", "linear"), loss="mse"), "2048")):
        rc, msg = _check(**kw)
        assert rc == E_INVALID and word in msg, (kw, rc, msg)
    lib = _lib.load()
    assert _check((1, 50, 1), ("relu", "linear"), "mse", k=10, batch=128, batch_size=128)[0] == 0    # D = 151
    assert _check((2, 8, 1), ("tanh", "linear"), "mse", batch=512, batch_size=512)[0] == 0           # n = 1024
    # a NULL plan and NULL systems are refused before the device is touched
    none = [None] * 3
    assert lib.pyz_fsvi_step(None, None, None, 1, None, None, None, None, None, 1, 1, None, None, 0.1, 1, 0, *none, *none,
                             None, None, None, None) == E_INVALID
    assert "null plan" in lib.pyz_last_error().decode()
    assert lib.pyz_spd_solve_f64(None, None, 4, 1, None, None) == E_INVALID
    fake = C.c_void_p(4096)
    for n, systems in ((0, 1), (2049, 1), (4, 0)):
        assert lib.pyz_spd_solve_f64(fake, fake, n, systems, None, None) == E_INVALID, (n, systems)
    assert _lib.header_version() == 302
