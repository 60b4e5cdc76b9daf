"""Device tests of visualisations.Plotter over BayesianModel.grid_surface / predictive_surface.

A ``Sampled`` posterior that holds ONE weight vector makes every draw that vector, so every surface has a float64 value:
the oracle forward of the vector on a grid built on the host in float64 (plotter_checks.grid_axes64, meshgrid 'ij',
``grid @ base_matrix^T``).  The device is held to rtol 1e-4 of the largest value, the bound tests/test_gpu_metrics.py
grants the forward; the uncertainty mask may differ only where |top - threshold| is inside that tolerance."""

import numpy as np
import pytest

from plotter_checks import grid_axes64, moons, summary
from oracle import mlp as o_mlp
from bayesian_inference_for_nn_amd.distributions import Sampled
from bayesian_inference_for_nn_amd.engine import KernelProbe
from bayesian_inference_for_nn_amd.nn import BayesianModel
from bayesian_inference_for_nn_amd.visualisations import Plotter
from bayesian_inference_for_nn_amd.visualisations.Plotter import confusion_counts, pca_axes

pytestmark = pytest.mark.gpu

RTOL = 1e-4
GRANULARITY, ROWS, THRESHOLD = 0.13, 80, 0.8


def _model(s):
    bm = BayesianModel(s.cfg)
    bm.apply_distribution(Sampled([s.theta], [1]), 0, 1)
    return bm


def _host_surface(s, x2, base64):
    """float64 probabilities (n1 * n2, 2) of the one weight vector on the host-built grid, and the grid's shape."""
    a0, da, n1, b0, db, n2 = grid_axes64(x2, GRANULARITY, 0.2)
    u, v = np.meshgrid(a0 + np.arange(n1) * da, b0 + np.arange(n2) * db, indexing="ij")
    grid = np.stack([u.reshape(-1), v.reshape(-1)], axis=1) @ base64.T
    return o_mlp.predict(s.theta, grid, s.spec), (n1, n2)


@pytest.mark.parametrize("d", [2, 5])
def test_surfaces_match_the_float64_read_out_of_a_host_grid(d, gpu_device):
    s = moons(d, ROWS)
    bm = _model(s)
    x, y = s.dataset.test_data.as_numpy()
    assert len(x) == ROWS
    x64 = np.asarray(x, dtype=np.float64)
    base64 = np.eye(2) if d == 2 else pca_axes(x64, 2)
    p, shape = _host_surface(s, x64 @ base64 if d > 2 else x64, base64)
    assert shape == (8, 8)
    tol = RTOL * np.abs(p).max()
    pl = Plotter(bm, s.dataset)

    with KernelProbe(256) as kp:
        ua = pl.uncertainty_area_data(granularity=GRANULARITY, n_samples=ROWS, uncertainty_threshold=THRESHOLD)
    names = [k for k, _ in kp.launches]
    assert names.count("k_grid_rows") == 1 and names.count("k_predict_surface") >= 1
    assert "k_predict_rows" not in names and "k_predict_mean" not in names
    assert ua["top"].shape == shape and ua["dim1"].shape == shape and ua["top"].dtype == np.float32
    np.testing.assert_array_equal(ua["base_matrix"], base64.astype(np.float32))
    top64 = p.max(axis=1).reshape(shape)
    diff = np.abs(ua["top"] - top64)
    print(f"d = {d}: max |top - float64| = {diff.max():.3e}, tolerance {tol:.3e}")
    assert diff.max() <= tol
    want = (top64 < THRESHOLD).astype(np.float32)
    clear = np.abs(top64 - THRESHOLD) > tol
    np.testing.assert_array_equal(ua["uncertain"][clear], want[clear])
    assert 0 < ua["uncertain"].sum() < ua["uncertain"].size         # both sides of the threshold occur
    assert list(ua["classes"]) == [0, 1]
    np.testing.assert_array_equal(bm._model.weights_flat, s.theta)  # the last draw is left assigned

    db = pl.decision_boundaries_data(granularity=GRANULARITY, n_boundaries=3, n_samples=ROWS)
    assert db["boundaries"].shape == (10,) + shape and db["n_boundaries"] == 10
    diff = np.abs(db["boundaries"] - p[:, 0].reshape(shape)[None])
    print(f"d = {d}: max |boundary column - float64| = {diff.max():.3e}")
    assert diff.max() <= tol
    assert p[:, 0].min() < 0.5 < p[:, 0].max()                      # the window holds a boundary

    # the grid in row chunks of 16: the bits of the unchunked read-out
    bm._predict_rows_cap = 16
    with KernelProbe(256) as kp:
        ua_c = pl.uncertainty_area_data(granularity=GRANULARITY, n_samples=ROWS, uncertainty_threshold=THRESHOLD)
    assert [k for k, _ in kp.launches].count("k_grid_rows") == 4
    db_c = pl.decision_boundaries_data(granularity=GRANULARITY, n_samples=ROWS)
    np.testing.assert_array_equal(ua_c["top"], ua["top"])
    np.testing.assert_array_equal(ua_c["uncertain"], ua["uncertain"])
    np.testing.assert_array_equal(db_c["boundaries"], db["boundaries"])


def test_entropy_and_confusion_matrix_agree_with_the_predictive_mean(gpu_device):
    s = moons(2, ROWS)
    bm = _model(s)
    x, y = s.dataset.test_data.as_numpy()
    mean = bm.predictive_mean(x, 4)
    pl = Plotter((bm, None), s.dataset)
    ent = pl.entropy_data(n_boundaries=4, n_samples=ROWS)
    _, cls, ent64, bound = summary(mean)
    assert ent.shape == (ROWS,) and (np.diff(ent) >= 0).all()
    assert np.abs(ent.astype(np.float64) - np.sort(ent64)).max() <= bound.max()
    labels, counts, norm = pl.confusion_matrix_data(n_boundaries=4, n_samples=ROWS)
    ref = confusion_counts(y, cls)
    np.testing.assert_array_equal(labels, ref[0])
    np.testing.assert_array_equal(counts, ref[1])
    np.testing.assert_array_equal(norm, ref[2])
    assert counts.sum() == ROWS and list(labels) == [0, 1]
    cols, smean, top, scls, _ = bm.predictive_surface(x, 4, column=1, want_cols=True)
    np.testing.assert_array_equal(smean, mean)
    np.testing.assert_array_equal(scls, cls)
    np.testing.assert_array_equal(top, mean.max(axis=1))
    assert cols.shape == (4, ROWS) and (cols == cols[0]).all()
    fpr, tpr, _ = pl.roc_data(n_samples=ROWS, label_of_interest=1, n_boundaries=4)
    assert fpr[0] == tpr[0] == 0.0 and fpr[-1] == tpr[-1] == 1.0
