"""Device tests of pyz_input_grad (k_input_grad, csrc/pyz_input_grad.h) against the float64 restatement of
tests/input_grad_checks.py, and of the surface above it: BayesianModel.adversarial_examples and
Robustness.adversarial_robustness.

Bounds.  The gradient is held to max |diff| <= 1e-4 max |ref|, the bound tests/test_gpu_dense_matrix.py applies to every
Dense kernel (float32 chains of a few hundred terms stay two orders below it).  The FGSM result depends on the SIGN of the
gradient only, so it is compared exactly where float32 cannot turn the sign -- |ref| > 1e-3 max |ref|, ten times the
gradient's own bound -- and held to |xadv - x| <= eps elsewhere; tests/test_input_grad_host.py caps the share of those
elements at 3 % on the reference of these very cases."""

import ctypes as C

import numpy as np
import pytest
import torch

from input_grad_checks import (CASES, EXCLUDE_CAP, accuracy, case_ref, fgsm, rmse, sign_stable, surface_classification,
                               surface_regression)
from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.distributions import Sampled
from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPPlan, MLPSpec
from bayesian_inference_for_nn_amd.losses import MeanSquaredError
from bayesian_inference_for_nn_amd.nn import BayesianModel
from bayesian_inference_for_nn_amd.visualisations import Robustness

pytestmark = pytest.mark.gpu

TOL = 1e-4
EPS = 0.125


def _dev(case, gpu_device):
    x, y, thetas, G, losses = case_ref(case)
    return (torch.tensor(x, device=gpu_device), torch.tensor(y, device=gpu_device), torch.tensor(thetas, device=gpu_device))


def _plan(case, max_p, gpu_device, extra_rows=0):
    return MLPPlan(MLPSpec(case.dims, case.acts, case.loss), max_batch=case.rows + extra_rows, max_particles=max_p,
                   device=gpu_device)


def _close(got, ref):
    diff, top = np.abs(got.astype(np.float64) - ref).max(), np.abs(ref).max()
    print(f"max |diff| = {diff:.3e}, max |ref| = {top:.3e}, ratio {diff / top:.3e}")
    return diff <= TOL * top


def _check_xadv(xadv, x, ref, eps):
    keep = sign_stable(ref)
    print(f"excluded share {1.0 - keep.mean():.4f}")
    assert 1.0 - keep.mean() <= EXCLUDE_CAP
    np.testing.assert_array_equal(xadv[keep], fgsm(x, ref, eps)[keep])
    # |xadv - x| <= eps on the rest, with the end points rounded as the device rounds them (x +- eps in float32)
    lo, hi = x - np.float32(eps), x + np.float32(eps)
    assert ((xadv[~keep] >= lo[~keep]) & (xadv[~keep] <= hi[~keep])).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gradient_losses_and_fgsm_match_the_restatement(case, gpu_device):
    x, y, thetas, G, losses = case_ref(case)
    xd, yd, wd = _dev(case, gpu_device)
    plan = _plan(case, case.max_p, gpu_device)
    with KernelProbe(64) as kp:
        g1, a1, l1 = plan.input_grad(wd, xd, yd, epsilon=EPS)
    names = [n for n, _ in kp.launches]
    assert names.count("k_input_grad") == len(case.launches())          # the library's own kernel ran, once per chunk
    g2, a2, l2 = plan.input_grad(wd, xd, yd, epsilon=EPS)
    plan.check_finite()
    assert _close(g1.cpu().numpy(), G)                                                      # (1)
    np.testing.assert_allclose(l1.cpu().numpy(), losses, rtol=1e-4)                         # (2)
    assert torch.equal(g1, g2) and torch.equal(a1, a2) and torch.equal(l1, l2)              # (3)
    _check_xadv(a1.cpu().numpy(), x, G, EPS)                                                # (6)
    gh, ah, _ = plan.input_grad(wd, xd, yd, scale=0.5)                                      # (5)
    assert ah is None
    assert torch.equal(gh, 0.5 * g1)


@pytest.mark.parametrize("case", [c for c in CASES if c.draws > 1], ids=lambda c: c.name)
def test_chunked_draws_agree_with_one_chunk(case, gpu_device):
    x, y, thetas, G, losses = case_ref(case)
    xd, yd, wd = _dev(case, gpu_device)
    small = case.max_p if case.max_p < case.draws else (case.draws + 1) // 2
    g_one, a_one, l_one = _plan(case, case.draws, gpu_device).input_grad(wd, xd, yd, epsilon=EPS)
    g_chk, a_chk, l_chk = _plan(case, small, gpu_device).input_grad(wd, xd, yd, epsilon=EPS)
    diff = (g_one - g_chk).abs().max().item()
    print(f"chunks of {small}: max |one - chunked| = {diff:.3e}")
    assert diff <= TOL * np.abs(G).max()                                                    # (4)
    assert _close(g_chk.cpu().numpy(), G)
    np.testing.assert_allclose(l_chk.cpu().numpy(), losses, rtol=1e-4)
    _check_xadv(a_chk.cpu().numpy(), x, G, EPS)


@pytest.mark.parametrize("name", ["one_layer", "deep", "wide_p4_vec", "d_in_1"])
def test_rows_past_n_stay_untouched(name, gpu_device):
    """The plan and the buffers hold three rows more than the call uses: those rows of xgrad and xadv keep their sentinel.
    (The outputs are contiguous (n, in): a store past column in - 1 would land in the next row, where (1) catches it, or,
    from the last row, in the sentinel rows.)"""
    case = {c.name: c for c in CASES}[name]
    x, y, thetas, G, losses = case_ref(case)
    n, K = case.rows, case.dims[0]
    plan = _plan(case, case.max_p, gpu_device, extra_rows=3)
    xd = torch.zeros((n + 3, K), device=gpu_device)
    xd[:n] = torch.tensor(x, device=gpu_device)
    yd, wd = torch.tensor(y, device=gpu_device), torch.tensor(thetas, device=gpu_device)
    SENT = -777.0
    gd, ad = torch.full((n + 3, K), SENT, device=gpu_device), torch.full((n + 3, K), SENT, device=gpu_device)
    ld = torch.full((case.draws + 2,), SENT, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(plan.lib.pyz_input_grad(plan.h, _lib.ptr(wd), case.draws, _lib.ptr(xd), _lib.ptr(yd), n, 1.0, _lib.ptr(gd),
                                       EPS, _lib.ptr(ad), _lib.ptr(ld), st))
    torch.cuda.synchronize()
    assert (gd[n:] == SENT).all() and (ad[n:] == SENT).all() and (ld[case.draws:] == SENT).all()
    assert _close(gd[:n].cpu().numpy(), G)
    _check_xadv(ad[:n].cpu().numpy(), x, G, EPS)
    # the optional outputs left out: the gradient alone, the same bits
    g2 = torch.full((n + 3, K), SENT, device=gpu_device)
    _lib.check(plan.lib.pyz_input_grad(plan.h, _lib.ptr(wd), case.draws, _lib.ptr(xd), _lib.ptr(yd), n, 1.0, _lib.ptr(g2),
                                       0.0, None, None, st))
    assert torch.equal(g2, gd)


def test_bad_arguments_are_refused(gpu_device):
    case = CASES[0]
    xd, yd, wd = _dev(case, gpu_device)
    plan = _plan(case, 1, gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.empty_like(xd)
    call = plan.lib.pyz_input_grad
    assert call(plan.h, _lib.ptr(wd), 1, _lib.ptr(xd), _lib.ptr(yd), case.rows + 1, 1.0, _lib.ptr(g), 0.0, None, None, st) < 0
    assert call(plan.h, _lib.ptr(wd), 0, _lib.ptr(xd), _lib.ptr(yd), case.rows, 1.0, _lib.ptr(g), 0.0, None, None, st) < 0
    assert call(plan.h, _lib.ptr(wd), 1, _lib.ptr(xd), _lib.ptr(yd), case.rows, 1.0, None, 0.0, None, None, st) < 0
    assert call(plan.h, None, 1, _lib.ptr(xd), _lib.ptr(yd), case.rows, 1.0, _lib.ptr(g), 0.0, None, None, st) < 0
    bad = MLPPlan(MLPSpec((5, 3), ("linear",), "scce"), max_batch=9, device=gpu_device)       # scce without softmax
    assert bad.lib.pyz_input_grad(bad.h, _lib.ptr(wd), 1, _lib.ptr(xd), _lib.ptr(yd), 9, 1.0, _lib.ptr(g), 0.0, None, None,
                                  st) < 0
    with pytest.raises(ValueError):
        plan.input_grad(wd[:, :-1].contiguous(), xd, yd)
    with pytest.raises((ValueError, TypeError)):
        plan.input_grad(wd, xd, yd.float())


# ---------------------------------------------------------------- the surface
def _wrap_adv(monkeypatch, bm, seen):
    real = bm.adversarial_examples

    def wrapped(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out

    monkeypatch.setattr(bm, "adversarial_examples", wrapped)


def _model(s):
    bm = BayesianModel(s.cfg)
    bm.apply_distribution(Sampled([s.theta], [1]), 0, 1)          # a deterministic posterior: every draw is theta
    return bm


def test_classification_surface(gpu_device, monkeypatch, capsys, tmp_path):
    s = surface_classification()
    bm = _model(s)
    assert accuracy(s, s.xv) == 100.0 and accuracy(s, fgsm(s.xv, s.G, s.eps)) < 100.0   # the restatement's verdict
    for cap in (16384, 11):                                     # one launch sequence, and row chunks of 11 + 11 + 8
        bm._predict_rows_cap = cap
        x_adv, x_grad = bm.adversarial_examples(s.xv, s.yv, "scce", s.eps, s.draws)
        assert x_adv.shape == s.xv.shape and _close(x_grad, s.G)
        _check_xadv(x_adv, s.xv, s.G, s.eps)
    seen = []
    _wrap_adv(monkeypatch, bm, seen)
    rb = Robustness((bm, None), s.dataset)
    v = rb.adversarial_robustness(epsilon=s.eps, nb_samples=s.draws)
    assert v == accuracy(s, seen[0][0]) and v < 100.0
    assert capsys.readouterr().out.endswith("Adversarial Robustness: " + str(v) + "%\n")
    print("adversarial accuracy", v)
    v2 = rb.adversarial_robustness(epsilon=s.eps, nb_samples=s.draws, save_path=str(tmp_path))
    assert v2 == v and (tmp_path / "report" / "robustness" / "adversarial_robustness.txt").read_text() == str(v)
    x, y = s.dataset.train_data.as_numpy()
    with pytest.raises(ValueError):
        Robustness(bm, Dataset((x, y), MeanSquaredError, "Classification", seed=4)).adversarial_robustness(nb_samples=2)


def test_regression_surface(gpu_device, monkeypatch, capsys, tmp_path):
    """The score is the RMSE of the device's float32 mean prediction: it is held to 1e-5 of the float64 oracle's on the
    same inputs (float32 forward passes of this size agree with float64 to a few 1e-7)."""
    s = surface_regression()
    bm = _model(s)
    assert rmse(s, fgsm(s.xv, s.G, s.eps)) > rmse(s, s.xv)
    x_adv, x_grad = bm.adversarial_examples(s.xv, s.yv, "mse", s.eps, s.draws)
    assert _close(x_grad, s.G)
    _check_xadv(x_adv, s.xv, s.G, s.eps)
    seen = []
    _wrap_adv(monkeypatch, bm, seen)
    rb = Robustness(bm, s.dataset)
    v = rb.adversarial_robustness(epsilon=s.eps, nb_samples=s.draws)
    assert v == pytest.approx(rmse(s, seen[0][0]), rel=1e-5) and v > rmse(s, s.xv)
    assert capsys.readouterr().out.endswith("Adversarial Robustness: " + str(v) + "\n")
    print("adversarial rmse", v)
    v2 = rb.adversarial_robustness(epsilon=s.eps, nb_samples=s.draws, save_path=str(tmp_path))
    assert (tmp_path / "report" / "robustness" / "adversarial_robustness.txt").read_text() == str(v2)
