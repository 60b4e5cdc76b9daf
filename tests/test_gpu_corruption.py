"""Device tests of pyz_corrupt_rows / pyz_score_rows (k_corrupt_rows, k_score_rows, csrc/pyz_corrupt.h) against the
float64 restatements of tests/corruption_checks.py, and of the surface above them: BayesianModel.corruption_scores and
Robustness's corruption measures.

Bounds.  Unquantised outputs are held, per element, to pixel_max * (corruption_checks.bound + OUT_TAIL): float32 rounding
of the operations involved, derived there.  Impulse noise is compared bit for bit with the float32 evaluation of its
pass-through (its decisions are comparisons of fp32-exact uniforms); shot noise is exact in its counts except on elements
whose uniform lies within AMBIGUOUS_EPS of a float64 CDF boundary, which may differ by one count and whose share
tests/test_corruption_host.py caps on these very inputs.  The quantised output is compared bit for bit with the floor and
channel mean applied in float32 to the device's own unquantised channels."""

import ctypes as C

import numpy as np
import pytest
import torch

import corruption_checks as cc
from bayesian_inference_for_nn_amd import _lib, engine
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.distributions import Sampled
from bayesian_inference_for_nn_amd.engine import KernelProbe
from bayesian_inference_for_nn_amd.losses import MeanSquaredError, SparseCategoricalCrossentropy
from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json
from bayesian_inference_for_nn_amd.visualisations import Robustness

pytestmark = pytest.mark.gpu

SEV = list(cc.SEVERITIES)
PIXEL_MAX = (255.0, 1.0)
IMAGE_KINDS = range(9)


def _rows(case, pm, gpu_device):
    x = cc.case_input(case, pm)
    return x, torch.tensor(x.reshape(case.n, -1), device=gpu_device)


def _run(xd, case, kind, pm, quantise, sev=SEV, ch=None):
    ch = case.ch if ch is None else ch
    return engine.corrupt_rows(xd, (case.h, case.w, ch), kind, sev, pixel_max=pm, quantise=quantise, seed=cc.SEED)


def _channel_bound(b, ch):
    """bound (n, h, w, 3) -> per output element: the channels' own, or their mean's."""
    return (b.mean(axis=-1, keepdims=True) if ch == 1 else b).reshape(len(b), -1)


# ---------------------------------------------------------------- 1. unquantised parity
@pytest.mark.parametrize("pm", PIXEL_MAX, ids=lambda p: f"pm{int(p)}")
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_unquantised_output_matches_the_float64_restatement(case, pm, gpu_device):
    x, xd = _rows(case, pm, gpu_device)
    for kind in IMAGE_KINDS:
        got = _run(xd, case, kind, pm, False).cpu().numpy()
        assert got.shape == (5, case.n, case.h * case.w * case.ch)
        for s, sev in enumerate(SEV):
            res = cc.corrupt(x, kind, sev, pm, cc.SEED)
            ref = cc.finish(res["value"], case.ch, pm, False)
            err = np.abs(got[s].astype(np.float64) - ref)
            tail = pm * cc.OUT_TAIL
            if kind == cc.IMPULSE:
                v32 = np.asarray(x, dtype=np.float32) / np.float32(pm)
                v32 = np.repeat(v32, 3, axis=3) if case.ch == 1 else v32
                want = np.where(res["flipped"], res["value"].astype(np.float32), v32)
                np.testing.assert_array_equal(got[s], cc.finish(want, case.ch, pm, False, dtype=np.float32))
                continue
            if kind == cc.SHOT:
                amb = res["dist"] <= cc.AMBIGUOUS_EPS
                amb = (amb.sum(axis=-1, keepdims=True) if case.ch == 1 else amb.astype(np.int64)).reshape(case.n, -1)
                share = float((amb > 0).mean())
                one_count = pm / cc.TABLE[cc.SHOT][sev - 1] / (3.0 if case.ch == 1 else 1.0)
                print(f"{case.name} shot sev {sev}: open share {share:.5f}, max err {err.max():.3e}")
                assert share <= cc.AMBIGUOUS_CAP
                assert (err <= tail + amb * one_count).all()
                continue
            bnd = pm * _channel_bound(cc.bound(kind, sev, res, res["value"].shape), case.ch) + tail
            print(f"{case.name} {cc.NAMES[kind]} sev {sev}: max err / bound = {float((err / bnd).max()):.3f}")
            assert (err <= bnd).all(), f"{cc.NAMES[kind]} severity {sev}: worst element at {float((err / bnd).max()):.3f} of its bound"


@pytest.mark.parametrize("rows,length", cc.ROW_CASES, ids=str)
def test_regression_noise_matches_the_float64_restatement(rows, length, gpu_device):
    x = cc.row_case_data(rows, length)
    xd = torch.tensor(x, device=gpu_device)
    got = engine.corrupt_rows(xd, (1, length, 1), cc.REGRESSION, SEV, pixel_max=123.0, quantise=True, seed=cc.SEED).cpu().numpy()
    for s, sev in enumerate(SEV):
        ref, z = cc.regression_noise(x, sev, cc.SEED)
        assert (np.abs(got[s] - ref) <= cc.regression_bound(x, sev, z)).all()       # (no clip, no quantisation, no scaling)


# ---------------------------------------------------------------- 2. quantised output, bit for bit
def _levels(out0, pm):
    """floor(255 v) in float32 from the unquantised channels out0 = float32(v * pixel_max): the same product for
    pixel_max = 255, and v itself for pixel_max = 1."""
    return np.floor(out0) if pm == 255.0 else np.floor(np.float32(255.0) * out0)


@pytest.mark.parametrize("pm", PIXEL_MAX, ids=lambda p: f"pm{int(p)}")
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_quantised_output_is_the_floor_of_the_devices_own_channels(case, pm, gpu_device):
    x, xd = _rows(case, pm, gpu_device)
    x3 = np.repeat(x, 3, axis=3) if case.ch == 1 else x          # the colour form of the same replicated image
    x3d = torch.tensor(x3.reshape(case.n, -1), device=gpu_device)
    scale = np.float32(pm) / np.float32(255.0)
    for kind in IMAGE_KINDS:
        got = _run(xd, case, kind, pm, True).cpu().numpy()
        chan = _run(x3d, case, kind, pm, False, ch=3).cpu().numpy().reshape(5, case.n, case.h * case.w, 3)
        lev = _levels(chan, pm)
        assert lev.min() >= 0 and lev.max() <= 255
        if case.ch == 1:
            want = (lev[..., 0] + lev[..., 1] + lev[..., 2]) / np.float32(3.0) * scale
        else:
            want = (lev * scale).reshape(5, case.n, -1)
        np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=cc.NAMES[kind])


# ---------------------------------------------------------------- 3. determinism and addressing
@pytest.mark.parametrize("case", [cc.CASES[1], cc.CASES[3], cc.CASES[5]], ids=lambda c: c.name)
def test_same_bits_again_per_severity_and_nothing_else_written(case, gpu_device):
    x, xd = _rows(case, 255.0, gpu_device)
    before = xd.clone()
    lib, st = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L, SENT = case.h * case.w * case.ch, -777.0
    for kind in IMAGE_KINDS:
        a = _run(xd, case, kind, 255.0, True)
        assert torch.equal(a, _run(xd, case, kind, 255.0, True))
        for s in (1, 5, 3):
            assert torch.equal(_run(xd, case, kind, 255.0, True, sev=[s])[0], a[s - 1])
        pair = _run(xd, case, kind, 255.0, True, sev=[4, 2])
        assert torch.equal(pair[0], a[3]) and torch.equal(pair[1], a[1])
        buf = torch.full((5 * case.n + 3, L), SENT, device=gpu_device)
        _lib.check(lib.pyz_corrupt_rows(_lib.ptr(xd), case.n, case.h, case.w, case.ch, kind, (C.c_int32 * 5)(*SEV), 5, 255.0, 1,
                                        cc.SEED, _lib.ptr(buf), st))
        assert torch.equal(buf[:5 * case.n].reshape(5, case.n, L), a) and (buf[5 * case.n:] == SENT).all()
    assert torch.equal(xd, before)


def test_regression_noise_addressing(gpu_device):
    rows, length = cc.ROW_CASES[2]
    xd = torch.tensor(cc.row_case_data(rows, length), device=gpu_device)
    before = xd.clone()
    a = engine.corrupt_rows(xd, (1, length, 1), cc.REGRESSION, SEV, seed=cc.SEED)
    assert torch.equal(a, engine.corrupt_rows(xd, (1, length, 1), cc.REGRESSION, SEV, seed=cc.SEED))
    assert torch.equal(engine.corrupt_rows(xd, (1, length, 1), cc.REGRESSION, [4], seed=cc.SEED)[0], a[3])
    assert not torch.equal(engine.corrupt_rows(xd, (1, length, 1), cc.REGRESSION, SEV, seed=cc.SEED + 1), a)
    buf = torch.full((5 * rows + 3, length), -777.0, device=gpu_device)
    _lib.check(_lib.load().pyz_corrupt_rows(_lib.ptr(xd), rows, 1, length, 1, cc.REGRESSION, (C.c_int32 * 5)(*SEV), 5, 255.0, 1,
                                            cc.SEED, _lib.ptr(buf), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(buf[:5 * rows].reshape(5, rows, length), a) and (buf[5 * rows:] == -777.0).all()
    assert torch.equal(xd, before)


def test_bad_arguments_are_refused(gpu_device):
    xd = torch.zeros((2, 64), device=gpu_device)
    with pytest.raises(ValueError):
        engine.corrupt_rows(xd, (8, 8, 1), 0, [0])
    with pytest.raises(ValueError):
        engine.corrupt_rows(xd, (8, 8, 1), 10, [1])
    with pytest.raises(ValueError):
        engine.corrupt_rows(xd, (8, 8, 3), 0, [1])
    with pytest.raises(_lib.PyzError):
        engine.corrupt_rows(torch.zeros((2, 128), device=gpu_device), (8, 8, 2), 0, [1])
    with pytest.raises(TypeError):
        engine.score_rows(torch.zeros((1, 2, 3), device=gpu_device), torch.zeros(2, device=gpu_device), 0)
    with pytest.raises(ValueError):
        engine.score_rows(torch.zeros((1, 2, 3), device=gpu_device), torch.zeros(5, device=gpu_device), 1)


# ---------------------------------------------------------------- 4. pyz_score_rows
def _score_classes(mean, y, gpu_device):
    got = engine.score_rows(torch.tensor(mean, device=gpu_device), torch.tensor(y, device=gpu_device), 0)
    assert got.dtype == torch.int64
    return got.cpu().numpy()


def test_classification_counts_equal_numpy(gpu_device):
    rng = np.random.default_rng(5)
    mean = rng.random((3, 257, 10)).astype(np.float32)
    mean[:, ::5, 7] = mean[:, ::5, 2] = 2.0            # exact ties of the maximum: the first index wins, as np.argmax
    mean[1, ::3] = 0.25                                # whole rows tied: class 0
    y = rng.integers(0, 10, size=257).astype(np.int32)
    y[::5] = np.where(np.arange(257)[::5] % 2 == 0, 2, 7)
    want = (mean.argmax(axis=2) != y[None]).sum(axis=1)
    assert 0 < want.min() and want.max() < 257
    np.testing.assert_array_equal(_score_classes(mean, y, gpu_device), want)
    one = np.array([[[0.5, 0.5]]], dtype=np.float32)   # C = 2, n = 1, a tie
    assert _score_classes(one, np.array([0], np.int32), gpu_device).tolist() == [0]
    assert _score_classes(one, np.array([1], np.int32), gpu_device).tolist() == [1]
    # C = 1: class 1 where the mean exceeds 0.5; exactly 0.5 is class 0
    p = np.array([0.1, 0.5, 0.9, np.nextafter(np.float32(0.5), np.float32(1.0)), 0.49999997, 0.7], dtype=np.float32)
    p = np.stack([p, 1 - p]).reshape(2, 6, 1)
    y1 = np.array([0, 0, 1, 1, 1, 0], dtype=np.int32)
    want = np.array([((g[:, 0] > 0.5).astype(np.int32) != y1).sum() for g in p])
    assert want.tolist() == [2, 4]
    np.testing.assert_array_equal(_score_classes(p, y1, gpu_device), want)


@pytest.mark.parametrize("C_out", [1, 3])
def test_regression_sums_match_float64(C_out, gpu_device):
    rng = np.random.default_rng(6 + C_out)
    mean = rng.normal(size=(2, 257, C_out)).astype(np.float32)
    y = rng.normal(size=(257, C_out)).astype(np.float32)
    md, yd = torch.tensor(mean, device=gpu_device), torch.tensor(y, device=gpu_device)
    got = engine.score_rows(md, yd, 1)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, C_out)
    term = (mean.astype(np.float64) - y[None].astype(np.float64)) ** 2
    err = np.abs(got.cpu().numpy() - term.sum(axis=1))
    assert (err <= 257 * 2.0 ** -53 * term.sum(axis=1)).all()
    assert torch.equal(got, engine.score_rows(md, yd, 1))
    # more than one workgroup of rows per group: the sums of the workgroups in order
    big = rng.normal(size=(2, 5000, C_out)).astype(np.float32)
    yb = rng.normal(size=(5000, C_out)).astype(np.float32)
    gb = engine.score_rows(torch.tensor(big, device=gpu_device), torch.tensor(yb, device=gpu_device), 1).cpu().numpy()
    tb = ((big.astype(np.float64) - yb[None]) ** 2).sum(axis=1)
    assert (np.abs(gb - tb) <= 5000 * 2.0 ** -53 * tb).all()


# ---------------------------------------------------------------- 5. end to end
def _deterministic_model(cfg, theta):
    bm = BayesianModel(cfg)
    bm.apply_distribution(Sampled([theta], [1]), 0, 1)            # every draw is theta
    return bm


def _classification_surface():
    from oracle import mlp as o_mlp
    rng = np.random.default_rng(41)
    spec = o_mlp.MLPSpec((64, 16, 4), ("tanh", "softmax"), "scce")
    theta = (0.05 * rng.normal(size=spec.n_params)).astype(np.float32)
    x = rng.integers(0, 256, size=(40, 8, 8)).astype(np.float32)
    y = o_mlp.predict(theta, x.reshape(40, -1), spec).argmax(axis=1).astype(np.int32)
    y[::6] = (y[::6] + 1) % 4                                       # (the clean error is not zero)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", train_proportion=0.0, test_proportion=0.0,
                 valid_proportion=1.0, seed=3)
    return _deterministic_model(sequential_json(64, [16, 4], ["tanh", "softmax"]), theta), ds


def test_corruption_errors_equal_the_host_scoring_of_the_devices_rows(gpu_device, capsys, tmp_path):
    bm, ds = _classification_surface()
    rb = Robustness(bm, ds, seed=77)
    xv, yv = ds.valid_data.as_numpy()
    assert xv.shape == (40, 8, 8)
    xd = torch.tensor(xv.reshape(40, -1), device=gpu_device)
    fractions = {}
    for kind, name in enumerate(cc.NAMES):
        with KernelProbe(256) as kp:
            v = rb.corruption_error(name, nb_boundaries=3, helper=True)
        names = [n for n, _ in kp.launches]
        assert names.count("k_corrupt_rows") == 1 and names.count("k_score_rows") == 1 and "k_predict_rows" not in names
        rows = engine.corrupt_rows(xd, (8, 8, 1), kind, SEV, pixel_max=255.0, quantise=True, seed=77)
        mean = bm.predictive_mean(rows.reshape(200, -1).cpu().numpy(), 3).reshape(5, 40, 4)
        fractions[name] = (mean.argmax(axis=2) != np.asarray(yv).reshape(1, -1)).mean(axis=1)
        assert v == np.sum(fractions[name] * 100) / 5, name
        np.testing.assert_array_equal(rb.error_dict[name], fractions[name])
    assert any(f.max() > 0 for f in fractions.values())
    clean = bm.predictive_mean(xv, 3)
    clean_error = 1.0 - float((clean.argmax(axis=1) == np.asarray(yv).reshape(-1)).mean())
    assert 0.0 < clean_error < 1.0
    capsys.readouterr()
    m = rb.mean_corruption_error(relative=True, nb_samples=3)
    assert m == pytest.approx(np.mean([np.sum(f * 100 - clean_error) / 5 for f in fractions.values()]), rel=1e-12)
    assert capsys.readouterr().out == "Mean Relative Error: " + str(m) + " %\n"
    nine = rb.robustness_by_corruption(nb_samples=3, save_path=str(tmp_path))
    np.testing.assert_allclose(nine, [np.sum(f * 100) / 5 for f in fractions.values()], rtol=1e-15)


def test_regression_branch_equals_the_host_rmse(gpu_device):
    from oracle import mlp as o_mlp
    rng = np.random.default_rng(43)
    spec = o_mlp.MLPSpec((11, 8, 1), ("tanh", "linear"), "mse")
    theta = (0.4 * rng.normal(size=spec.n_params)).astype(np.float32)
    x = rng.normal(size=(30, 11)).astype(np.float32)
    y = (o_mlp.predict(theta, x, spec) + 0.1 * rng.normal(size=(30, 1))).astype(np.float32)
    ds = Dataset((x, y), MeanSquaredError, "Regression", target_dim=1, train_proportion=0.0, test_proportion=0.0,
                 valid_proportion=1.0, seed=4)
    bm = _deterministic_model(sequential_json(11, [8, 1], ["tanh", "linear"]), theta)
    rb = Robustness(bm, ds, seed=12)
    xv, yv = ds.valid_data.as_numpy()
    with KernelProbe(256) as kp:
        v = rb.corruption_error(helper=True, nb_boundaries=2)
    names = [n for n, _ in kp.launches]
    assert names.count("k_corrupt_rows") == 1 and names.count("k_score_rows") == 1 and names.count("k_score_sum") == 1
    rows = engine.corrupt_rows(torch.tensor(np.asarray(xv, dtype=np.float32), device=gpu_device), (1, 11, 1), cc.REGRESSION, SEV,
                               seed=12)
    mean = bm.predictive_mean(rows.reshape(150, -1).cpu().numpy(), 2).reshape(5, 30, 1).astype(np.float64)
    rmse = np.sqrt(((mean - np.asarray(yv, dtype=np.float64).reshape(1, 30, 1)) ** 2).mean(axis=1)).mean(axis=1)
    assert v == pytest.approx(rmse.sum() / 5, rel=1e-6)
