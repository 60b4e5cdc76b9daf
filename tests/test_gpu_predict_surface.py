"""Device tests of pyz_grid_rows and pyz_predict_surface (k_grid_rows, k_predict_surface: csrc/pyz_surface.h) over the
case table of tests/plotter_checks.py.

pyz_grid_rows: bit for bit against the NumPy float32 restatement; the rows after a window keep their sentinel.

What each case holds pyz_predict_surface to, for columns 0 and C - 1:
  (1) d_mean is pyz_predict's mean and d_cols its column, bit for bit;
  (2) top and cls are NumPy's max / argmax of that float32 mean, exactly (one output: of the pair (1 - m, m));
  (3) ent against the float64 formula on the float32 mean, within
      |diff| <= 2^-24 ((C + 3) sum_a |q_a log(q_a + c)| + 2 sum_a |q_a|), c = float32(1e-5) (plotter_checks.summary:
      derived from float32 rounding, not measured); NaN where the formula is NaN (a negative mean of a linear layer);
  (4) a second call gives the same bits, and so does the other chunking of the draws;
  (5) the plan and the output buffers hold three rows more than the call uses: those keep their sentinel;
  (6) k_predict_surface ran once per chunk, and neither k_predict_rows nor k_predict_mean did."""

import ctypes as C

import numpy as np
import pytest
import torch

from plotter_checks import CASES, case_data, grid_rows_f32, pair, summary
from bayesian_inference_for_nn_amd import _lib, engine
from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPPlan, MLPSpec

pytestmark = pytest.mark.gpu

SENT = -777.0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- pyz_grid_rows
GRID = dict(a0=-1.37, da=0.2113, n1=7, b0=0.4021, db=0.0917, n2=5)


@pytest.mark.parametrize("d", [2, 5])
@pytest.mark.parametrize("row0,n", [(0, 35), (11, 17)], ids=["whole", "window"])
def test_grid_rows_equal_the_float32_restatement(d, row0, n, gpu_device):
    basis = np.eye(2, dtype=np.float32) if d == 2 else np.random.default_rng(6).normal(size=(d, 2)).astype(np.float32)
    bd = torch.tensor(basis, device=gpu_device)
    out = torch.full((n + 3, d), SENT, device=gpu_device)
    _lib.check(_lib.load().pyz_grid_rows(_lib.ptr(bd), d, GRID["a0"], GRID["da"], GRID["n1"], GRID["b0"], GRID["db"],
                                         GRID["n2"], row0, n, _lib.ptr(out), _stream()))
    torch.cuda.synchronize()
    want = grid_rows_f32(basis, row0=row0, n=n, **GRID)
    assert want.shape == (n, d) and want.dtype == np.float32
    np.testing.assert_array_equal(out[:n].cpu().numpy(), want)
    assert (out[n:] == SENT).all()
    got = engine.grid_rows(bd, GRID["a0"], GRID["da"], GRID["n1"], GRID["b0"], GRID["db"], GRID["n2"], row0, n)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if d == 2:      # the identity basis: the rows are (u_i, v_j) in 'ij' order
        u = np.float32(GRID["a0"]) + np.arange(7, dtype=np.float32) * np.float32(GRID["da"])
        v = np.float32(GRID["b0"]) + np.arange(5, dtype=np.float32) * np.float32(GRID["db"])
        mesh = np.stack([m.reshape(-1) for m in np.meshgrid(u, v, indexing="ij")], axis=1)
        np.testing.assert_array_equal(want, mesh[row0:row0 + n])


def test_grid_rows_refuses_bad_arguments(gpu_device):
    bd = torch.eye(2, device=gpu_device)
    out = torch.empty((40, 2), device=gpu_device)
    call = _lib.load().pyz_grid_rows
    good = (_lib.ptr(bd), 2, 0.0, 0.1, 7, 0.0, 0.1, 5, 0, 35, _lib.ptr(out), _stream())
    assert call(*good) == 0
    for k, v in ((0, None), (10, None), (1, 0), (4, 0), (7, 0), (8, -1), (9, 0), (9, 36), (8, 30)):
        bad = list(good)
        bad[k] = v
        assert call(*bad) == -1, (k, v)
    with pytest.raises(ValueError):
        engine.grid_rows(bd, 0.0, 0.1, 7, 0.0, 0.1, 5, 30, 6)
    with pytest.raises(ValueError):
        engine.grid_rows(torch.eye(3, device=gpu_device), 0.0, 0.1, 7, 0.0, 0.1, 5)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- pyz_predict_surface
def _plan(case, max_p, gpu_device):
    return MLPPlan(MLPSpec(case.dims, case.spec.acts, case.spec.loss), max_batch=case.n + 3, max_particles=max_p,
                   device=gpu_device)


def _raw(plan, case, wd, xd, column, gpu_device):
    """pyz_predict_surface into buffers with three sentinel rows (cols: three sentinel values) after the call's."""
    n, Cc, S = case.n, case.C, case.draws
    cols = torch.full((S * n + 3,), SENT, device=gpu_device)
    mean = torch.full((n + 3, Cc), SENT, device=gpu_device)
    top = torch.full((n + 3,), SENT, device=gpu_device)
    cls = torch.full((n + 3,), -777, dtype=torch.int32, device=gpu_device)
    ent = torch.full((n + 3,), SENT, device=gpu_device)
    _lib.check(plan.lib.pyz_predict_surface(plan.h, _lib.ptr(wd), S, _lib.ptr(xd), n, column, _lib.ptr(cols), _lib.ptr(mean),
                                            _lib.ptr(top), _lib.ptr(cls), _lib.ptr(ent), _stream()))
    torch.cuda.synchronize()
    return cols, mean, top, cls, ent


def _same(a, b):
    """bit equality of two tuples of tensors (NaN entropies of a linear layer included)."""
    return all(torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0)) if x.is_floating_point()
               else torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_surface_of_a_case(case, gpu_device):
    x, thetas = case_data(case)
    xd, wd = torch.tensor(x, device=gpu_device), torch.tensor(thetas, device=gpu_device)
    n, S = case.n, case.draws
    plan = _plan(case, case.max_p, gpu_device)          # the chunked plan
    whole = _plan(case, S, gpu_device)                  # every draw in one chunk
    samples, pmean = whole.predict(wd, xd)
    for column in sorted({0, case.C - 1}):
        with KernelProbe(64) as kp:
            out = _raw(plan, case, wd, xd, column, gpu_device)
        cols, mean, top, cls, ent = out
        names = [k for k, _ in kp.launches]
        assert names.count("k_predict_surface") == case.chunks                                  # (6)
        assert "k_predict_rows" not in names and "k_predict_mean" not in names
        assert (cols[S * n:] == SENT).all() and (mean[n:] == SENT).all() and (top[n:] == SENT).all()      # (5)
        assert (cls[n:] == -777).all() and (ent[n:] == SENT).all()
        assert torch.equal(mean[:n], pmean)                                                     # (1)
        assert torch.equal(cols[:S * n].reshape(S, n), samples[:, :, column])
        mean32 = mean[:n].cpu().numpy()
        ref_top, ref_cls, ref_ent, bound = summary(mean32)
        np.testing.assert_array_equal(top[:n].cpu().numpy(), ref_top)                           # (2)
        np.testing.assert_array_equal(cls[:n].cpu().numpy(), ref_cls)
        got_ent = ent[:n].cpu().numpy().astype(np.float64)
        nan = np.isnan(ref_ent)
        assert (np.isnan(got_ent) == nan).all()
        diff = np.abs(got_ent - ref_ent)[~nan]
        if diff.size:
            ratio = np.divide(diff, bound[~nan], out=np.zeros_like(diff), where=bound[~nan] > 0)
            print(f"column {column}: max |ent - float64| = {diff.max():.3e}, worst diff / bound = {ratio.max():.3f}")
            if (diff > bound[~nan]).any():      # what logf was given in the worst row
                print("logf inputs of the worst row:", pair(mean32)[~nan][int(np.argmax(ratio))] + np.float32(1e-5))
            assert (diff <= bound[~nan]).all()                                                  # (3)
        assert _same(_raw(plan, case, wd, xd, column, gpu_device), out)                         # (4)
        assert _same(_raw(whole, case, wd, xd, column, gpu_device), out)
        if case.nan_draw >= 0:      # the draw with the NaN weight counts as zeros
            assert torch.isfinite(mean[:n]).all() and (cols[:S * n].reshape(S, n)[case.nan_draw] == 0).all()
        # the engine's method: the same bits, without and with the optional outputs
        e_cols, e_mean, e_top, e_cls, e_ent = plan.predict_surface(wd, xd, column=column)
        assert e_cols.shape == (S, n) and e_mean.shape == (n, case.C) and e_cls.dtype == torch.int32
        assert _same((e_cols.reshape(-1), e_mean, e_top, e_cls, e_ent), (cols[:S * n], mean[:n], top[:n], cls[:n], ent[:n]))
        bare = plan.predict_surface(wd, xd, column=column, want_cols=False, want_summary=False)
        assert bare[0] is None and bare[2] is None and bare[3] is None and bare[4] is None and torch.equal(bare[1], mean[:n])
    plan.close()
    whole.close()


def test_bad_arguments_are_refused(gpu_device):
    case = CASES[1]                                     # 2 -> 8 -> 2, five draws
    assert case.dims == (2, 8, 2) and case.draws == 5
    x, thetas = case_data(case)
    xd, wd = torch.tensor(x, device=gpu_device), torch.tensor(thetas, device=gpu_device)
    plan = _plan(case, 2, gpu_device)
    n, S = case.n, case.draws
    mean = torch.empty((n + 4, case.C), device=gpu_device)
    call = plan.lib.pyz_predict_surface
    good = [plan.h, _lib.ptr(wd), S, _lib.ptr(xd), n, 0, None, _lib.ptr(mean), None, None, None, _stream()]
    assert call(*good) == 0                             # every optional output left out
    for k, v, code in ((4, n + 4, -2), (5, case.C, -1), (5, -1, -1), (2, 0, -1), (4, 0, -1), (7, None, -1), (1, None, -1),
                       (3, None, -1), (0, None, -1)):
        bad = list(good)
        bad[k] = v
        assert call(*bad) == code, (k, v)
    with pytest.raises(ValueError):
        plan.predict_surface(wd[:, :-1].contiguous(), xd)
    with pytest.raises(ValueError):
        plan.predict_surface(wd, xd[:, :-1].contiguous())
    with pytest.raises(ValueError):
        plan.predict_surface(wd, xd, column=case.C)
    with pytest.raises(ValueError):
        plan.predict_surface(wd, torch.zeros((n + 4, case.dims[0]), device=gpu_device))
    plan.close()
    # a row that does not fit the kernel's LDS: PYZ_E_SHAPE, as pyz_predict_moments answers it
    wide = MLPPlan(MLPSpec((2, 14000), ("linear",), "mse"), max_batch=1, max_particles=1, device=gpu_device)
    w = torch.zeros((1, wide.D), device=gpu_device)
    out = torch.empty((1, 14000), device=gpu_device)
    rc = wide.lib.pyz_predict_surface(wide.h, _lib.ptr(w), 1, _lib.ptr(xd), 1, 0, None, _lib.ptr(out), None, None, None, _stream())
    assert rc == -2 and "LDS" in wide.lib.pyz_last_error().decode()
    wide.close()
    torch.cuda.synchronize()
