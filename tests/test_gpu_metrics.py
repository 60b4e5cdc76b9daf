"""Device tests of visualisations.Metrics over BayesianModel.predictive_moments / predictive_mean.

A ``Sampled`` posterior that holds ONE weight vector makes every draw that vector, so each metric has a float64 value: the
host formulas of Metrics.py (pinned to sklearn, the reference's loop and a worked table by tests/test_metrics_host.py)
applied to the float64 oracle forward of the vector.  Metrics that count rows (accuracy, recall, precision, F1) and those
that rank or bin them (AUROC, ECE) are exact up to float64 rounding -- tests/test_metrics_host.py checks that the data keep
float32 away from every argmax, rank and bin edge; the others are held to rtol 1e-4, the bound of the Dense tests."""

import numpy as np
import pytest

from metrics_checks import surface_classification, surface_regression
from oracle import mlp as o_mlp
from bayesian_inference_for_nn_amd.distributions import Sampled
from bayesian_inference_for_nn_amd.engine import KernelProbe
from bayesian_inference_for_nn_amd.nn import BayesianModel
from bayesian_inference_for_nn_amd.visualisations import Metrics
from bayesian_inference_for_nn_amd.visualisations.Metrics import (accuracy_score, expected_calibration_error,
                                                                  gaussian_log_likelihood, macro_f1, macro_recall,
                                                                  mean_absolute_error, mean_squared_error, micro_auroc,
                                                                  micro_precision, r2_score, root_mean_squared_error,
                                                                  uncertainty_from_moments)

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def _model(s, last_layer):
    bm = BayesianModel(s.cfg)
    bm.apply_distribution(Sampled(list(s.thetas), [1] * len(s.thetas)), 0, last_layer)
    return bm


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    diff, top = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}: max |diff| = {diff:.3e}, max |ref| = {top:.3e}")
    assert diff <= RTOL * top, what


def test_classification_metrics_match_the_float64_forward(gpu_device, capsys, tmp_path):
    s = surface_classification()
    bm = _model(s, 1)
    x, y = s.dataset.test_data.as_numpy()
    rows, draws = 60, 5
    assert len(x) == rows
    p = o_mlp.predict(s.thetas[0], x, s.spec)
    pred = p.argmax(axis=1)
    m = Metrics(bm, s.dataset)
    out = m.summary(n_boundaries=draws, n_samples=rows, save_path=str(tmp_path))
    assert out["accuracy"] == accuracy_score(y, pred) * 100 and 50 < out["accuracy"] < 100
    assert out["precision"] == macro_recall(y, pred) * 100
    assert out["recall"] == micro_precision(y, pred) * 100
    assert out["f1_score"] == macro_f1(y, pred)
    assert out["auroc"] == pytest.approx(micro_auroc(y, p), rel=1e-12)
    assert out["ece"] == pytest.approx(expected_calibration_error(5, p, y), rel=RTOL)
    assert m.ece(n_boundaries=draws, n_samples=rows, n_bins=3) == pytest.approx(expected_calibration_error(3, p, y), rel=RTOL)
    assert (tmp_path / "report" / "Accuracy").read_text() == str(out["accuracy"])
    assert f"Accuracy: {out['accuracy']}%" in capsys.readouterr().out
    got = m.classification_uncertainty(n_boundaries=draws, n_samples=rows)
    want = uncertainty_from_moments(p, draws * np.einsum("ja,jb->jab", p, p), draws, rows)
    for g, w, what in zip(got, want, ("total", "aleatoric", "epistemic")):
        assert g.shape == (rows, 2, 2) and g.dtype == np.float64
        _close(g, w, what)
    # the first n_samples rows of the split
    assert m.accuracy(n_boundaries=draws, n_samples=17) == accuracy_score(y[:17], pred[:17]) * 100
    # predictive_moments' mean is predict's (the same draws: the posterior has one vector)
    mean, m2, nb = bm.predictive_moments(x, draws)
    _, pmean = bm.predict(x, draws)
    assert nb == draws and mean.dtype == np.float32 and m2.shape == (rows, 2, 2)
    np.testing.assert_array_equal(mean, np.asarray(pmean))
    bm._predict_rows_cap = 23                                   # row chunks of 23 + 23 + 14, joined on the device
    mean_c, m2_c, _ = bm.predictive_moments(x, draws)
    np.testing.assert_array_equal(mean_c, mean)
    np.testing.assert_array_equal(m2_c, m2)
    np.testing.assert_array_equal(bm._model.weights_flat, s.thetas[0])     # the last draw is left assigned


def test_regression_metrics_match_the_float64_forward(gpu_device, capsys):
    s = surface_regression()
    bm = _model(s, 0)
    x, y = s.dataset.test_data.as_numpy()
    p = o_mlp.predict(s.thetas[0], x, s.spec)
    m = Metrics((bm, None), s.dataset)
    with KernelProbe(64) as kp:
        out = m.summary(n_boundaries=4, n_samples=50)
    names = [k for k, _ in kp.launches]
    assert "k_predict_mean" in names and "k_predict_moments" not in names        # the mean-only read-out, once
    assert names.count("k_predict_mean") == 1
    want = {"mse": mean_squared_error(y, p), "rmse": root_mean_squared_error(y, p), "mae": mean_absolute_error(y, p),
            "r2": r2_score(y, p), "log_likeliood": gaussian_log_likelihood(y, p)}
    assert list(out) == list(want)
    for k in want:
        print(k, out[k], want[k])
        assert out[k] == pytest.approx(want[k], rel=RTOL), k
    assert 0.5 < out["r2"] < 1.0
    assert capsys.readouterr().out.count("\n") >= 5
    with pytest.raises(Exception):
        m.accuracy()


def test_uncertainty_of_a_posterior_of_several_vectors(gpu_device, monkeypatch):
    s = surface_classification(k=4)
    bm = _model(s, 1)
    seen = []
    real = bm.predictive_moments

    def wrapped(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out

    monkeypatch.setattr(bm, "predictive_moments", wrapped)
    m = Metrics(bm, s.dataset)
    rows, draws = 60, 9
    with KernelProbe(64) as kp:
        total, alea, epi = m.classification_uncertainty(n_boundaries=draws, n_samples=rows)
    assert [k for k, _ in kp.launches].count("k_predict_moments") == 1 and len(seen) == 1
    mean, m2, nb = seen[0]
    assert nb == draws
    # the draws differ: the second moment is not the outer product of the mean
    outer = draws * np.einsum("ja,jb->jab", mean.astype(np.float64), mean.astype(np.float64))
    assert np.abs(m2 - outer).max() > 1e-3
    want = uncertainty_from_moments(mean, m2, draws, rows)
    for g, w in zip((total, alea, epi), want):
        np.testing.assert_array_equal(g, w)
    np.testing.assert_allclose(total, alea + epi, rtol=0, atol=1e-12 * np.abs(total).max())
    # the probabilities of a row sum to 1, so each matrix row of a per-row aleatoric term diag(S1) - S2 sums to
    # S1_a - sum_s p_a sum_b p_b = 0 (float32 sums of nine draws: far inside 1e-4)
    np.testing.assert_allclose(np.diff(np.concatenate([np.zeros((1, 2, 2)), alea]), axis=0).sum(axis=2), 0.0, atol=1e-4)
    with KernelProbe(64) as kp:
        again = m.classification_uncertainty(n_boundaries=draws, n_samples=rows)
        acc = m.accuracy(n_boundaries=draws, n_samples=rows)
    assert kp.launches == [] and len(seen) == 1                 # a hit: nothing ran on the device
    np.testing.assert_array_equal(again[0], total)
    assert 0.0 <= acc <= 100.0


def test_the_compat_path_hands_out_the_library_class(gpu_device, monkeypatch):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "compat"))
    for name in [n for n in sys.modules if n == "Pyesian" or n.startswith("Pyesian.")]:
        monkeypatch.delitem(sys.modules, name)
    from Pyesian.visualisations import Metrics as compat_metrics
    assert compat_metrics is Metrics
    for name in [n for n in sys.modules if n == "Pyesian" or n.startswith("Pyesian.")]:
        sys.modules.pop(name, None)
