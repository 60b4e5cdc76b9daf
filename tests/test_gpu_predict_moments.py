"""Device tests of pyz_predict_moments (k_predict_moments, csrc/pyz_predict_moments.h) over the case table of
tests/metrics_checks.py (the issue's table, and three cases of more than 256 outputs, where the kernel takes its other path).

What each case holds the kernel to:
  (1) mean is pyz_predict's mean, bit for bit;
  (2) m2 against the float64 moments of the DEVICE'S OWN predict samples (the forward is not under test here), within
      the sequential-sum bound |diff| <= (S + 1) 2^-24 sum_s |p_a p_b| + 1e-30 per element (metrics_checks.m2_bound:
      derived from float32 rounding, not measured);
  (3) a second call gives the same bits;
  (4) draws chunked by a smaller max_particles give the bits of one chunk;
  (5) the plan and the output buffers hold three rows more than the call uses: those rows keep their sentinel;
  (6) k_predict_moments ran once per chunk, and neither k_predict_rows nor k_predict_mean did;
  (7) m2 is symmetric bit for bit."""

import ctypes as C

import numpy as np
import pytest
import torch

from metrics_checks import CASES, WIDE_CASES, case_data, m2_bound, moments
from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPPlan, MLPSpec

pytestmark = pytest.mark.gpu

SENT = -777.0


def _plan(case, max_p, gpu_device):
    return MLPPlan(MLPSpec(case.dims, case.spec.acts, case.spec.loss), max_batch=case.n + 3, max_particles=max_p,
                   device=gpu_device)


def _raw(plan, case, wd, xd, gpu_device):
    """pyz_predict_moments into buffers of n + 3 sentinel rows."""
    n, Cc = case.n, case.C
    mean = torch.full((n + 3, Cc), SENT, device=gpu_device)
    m2 = torch.full((n + 3, Cc, Cc), SENT, device=gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(plan.lib.pyz_predict_moments(plan.h, _lib.ptr(wd), case.draws, _lib.ptr(xd), n, _lib.ptr(mean), _lib.ptr(m2), st))
    torch.cuda.synchronize()
    return mean, m2


@pytest.mark.parametrize("case", CASES + WIDE_CASES, ids=lambda c: c.name)
def test_moments_of_a_case(case, gpu_device):
    x, thetas = case_data(case)
    xd, wd = torch.tensor(x, device=gpu_device), torch.tensor(thetas, device=gpu_device)
    plan = _plan(case, case.max_p, gpu_device)
    samples, pmean = plan.predict(wd, xd)
    with KernelProbe(64) as kp:
        mean, m2 = _raw(plan, case, wd, xd, gpu_device)
    names = [k for k, _ in kp.launches]
    assert names.count("k_predict_moments") == case.chunks                                  # (6)
    assert "k_predict_rows" not in names and "k_predict_mean" not in names
    n = case.n
    assert (mean[n:] == SENT).all() and (m2[n:] == SENT).all()                              # (5)
    assert torch.equal(mean[:n], pmean)                                                     # (1)
    ref_mean, ref_m2, abs2 = moments(samples.cpu().numpy())
    diff = np.abs(m2[:n].cpu().numpy().astype(np.float64) - ref_m2)
    bound = m2_bound(case.draws, abs2)
    print(f"max |m2 - float64| = {diff.max():.3e}, worst diff / bound = {(diff / bound).max():.3f}, "
          f"max |m2| = {np.abs(ref_m2).max():.3e}")
    assert (diff <= bound).all()                                                            # (2)
    assert torch.equal(m2[:n], m2[:n].transpose(1, 2))                                      # (7)
    mean_b, m2_b = _raw(plan, case, wd, xd, gpu_device)
    assert torch.equal(mean_b, mean) and torch.equal(m2_b, m2)                              # (3)
    if case.nan_draw >= 0:      # the draw with the NaN weight counts as zeros: a finite result, not a NaN one
        assert torch.isfinite(mean[:n]).all() and torch.isfinite(m2[:n]).all()
        assert (samples[case.nan_draw] == 0).all()
    # the other chunking: one chunk where the case is chunked, two chunks where it is not
    other_p = case.draws if case.chunks > 1 else max(1, (case.draws + 1) // 2)
    other = _plan(case, other_p, gpu_device)
    mean_o, m2_o = _raw(other, case, wd, xd, gpu_device)
    assert torch.equal(mean_o, mean) and torch.equal(m2_o, m2)                              # (4)
    # the engine's method: the same bits, (n, C) and (n, C, C)
    mean_e, m2_e = plan.predict_moments(wd, xd)
    assert mean_e.shape == (n, case.C) and m2_e.shape == (n, case.C, case.C)
    assert torch.equal(mean_e, mean[:n]) and torch.equal(m2_e, m2[:n])
    plan.close()
    other.close()


def test_bad_arguments_are_refused(gpu_device):
    case = CASES[5]
    x, thetas = case_data(case)
    xd, wd = torch.tensor(x, device=gpu_device), torch.tensor(thetas, device=gpu_device)
    plan = _plan(case, 2, gpu_device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mean = torch.empty((case.n + 4, case.C), device=gpu_device)
    m2 = torch.empty((case.n + 4, case.C, case.C), device=gpu_device)
    call = plan.lib.pyz_predict_moments
    assert call(plan.h, _lib.ptr(wd), case.draws, _lib.ptr(xd), case.n + 4, _lib.ptr(mean), _lib.ptr(m2), st) < 0   # n > max_batch
    assert call(plan.h, _lib.ptr(wd), case.draws, _lib.ptr(xd), case.n, _lib.ptr(mean), None, st) < 0               # null d_m2
    assert call(plan.h, _lib.ptr(wd), 0, _lib.ptr(xd), case.n, _lib.ptr(mean), _lib.ptr(m2), st) < 0                # n_samples = 0
    assert call(plan.h, _lib.ptr(wd), case.draws, _lib.ptr(xd), 0, _lib.ptr(mean), _lib.ptr(m2), st) < 0
    assert call(plan.h, _lib.ptr(wd), case.draws, _lib.ptr(xd), case.n, None, _lib.ptr(m2), st) < 0
    assert call(plan.h, None, case.draws, _lib.ptr(xd), case.n, _lib.ptr(mean), _lib.ptr(m2), st) < 0
    assert call(plan.h, _lib.ptr(wd), case.draws, _lib.ptr(xd), case.n, _lib.ptr(mean), _lib.ptr(m2), st) == 0
    with pytest.raises(ValueError):
        plan.predict_moments(wd[:, :-1].contiguous(), xd)
    with pytest.raises(ValueError):
        plan.predict_moments(wd, xd[:, :-1].contiguous())
    plan.close()
