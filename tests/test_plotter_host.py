"""CPU checks of the decision-surface entry points and of visualisations.Plotter: the two C-ABI rows and their argument
errors, the host restatements of Plotter.py (grid, PCA, ROC, confusion matrix) against float64, NumPy and sklearn, and the
bookkeeping of the class -- exceptions, the cache rule, the reference's quirks, the PNG files -- over a stubbed model."""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import plotter_checks as pc
from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.datasets.Dataset import ArrayDataset
from bayesian_inference_for_nn_amd.visualisations import Metrics, Plotter
from bayesian_inference_for_nn_amd.visualisations.Metrics import micro_auroc
from bayesian_inference_for_nn_amd.visualisations.Plotter import (confusion_counts, grid_axes, grid_mesh, pca_axes,
                                                                  pca_transform, roc_curve)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

CTYPE = {"const float *": _lib._p, "float *": _lib._p, "void *": _lib._p, "pyz_mlp *": _lib._p, "int32_t *": _lib._p,
         "int": C.c_int, "float": _lib._f, "int64_t": _lib._i64}


# ---------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("name,count", [("pyz_grid_rows", 12), ("pyz_predict_surface", 12)])
def test_entry_points_are_declared_with_matching_argument_types(name, count):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pyz.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert proto, f"{name} is not declared in include/pyz.h"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    types = [re.sub(r"\s*\w+$", "", p) for p in params]
    types = [t if not t.endswith("*") else t[:-1].strip() + " *" for t in types]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int
    assert [CTYPE[t] for t in types] == list(argtypes) and len(argtypes) == count
    assert hasattr(_lib.load(), name)
    assert _lib.header_version() == 302
    api = open(os.path.join(ROOT, "bayesian_inference_for_nn_amd", "csrc", "pyz_api.hip")).read()
    assert '#include "pyz_surface.h"' in api


def test_argument_errors_need_no_gpu():
    lib = _lib.load()
    good = dict(d=2, n1=7, n2=5, row0=0, n=35)
    for kw, word in ((dict(n1=0), "positive"), (dict(n2=0), "positive"), (dict(d=0), "positive"), (dict(n=0), "outside"),
                     (dict(row0=-1), "outside"), (dict(row0=30, n=6), "outside"), (dict(n=36), "outside"),
                     (dict(row0=36, n=1), "outside"), (dict(), "null device pointer")):
        a = dict(good, **kw)
        rc = lib.pyz_grid_rows(None, a["d"], 0.0, 0.1, a["n1"], 0.0, 0.1, a["n2"], a["row0"], a["n"], None, None)
        assert rc == E_INVALID and word in lib.pyz_last_error().decode(), (kw, lib.pyz_last_error())
    assert lib.pyz_predict_surface(None, None, 1, None, 1, 0, None, None, None, None, None, None) == E_INVALID
    assert "null plan" in lib.pyz_last_error().decode()


# ---------------------------------------------------------------- the grid
@pytest.mark.parametrize("granularity,count", [(0.13, 8), (0.21, 5), (0.3, 4)])
@pytest.mark.parametrize("ranges", [((-1.3, 2.2), (0.01, 0.02)), ((-50.0, 70.0), (-1.3, 2.2)), ((0.01, 0.02), (-50.0, 70.0))], ids=str)
def test_grid_extents_and_counts_equal_float64(granularity, count, ranges):
    rng = np.random.default_rng(12)
    x = np.stack([np.r_[lo, hi, rng.uniform(lo, hi, size=30)] for lo, hi in ranges], axis=1).astype(np.float32)
    got, want = grid_axes(x, granularity, 0.2), pc.grid_axes64(x, granularity, 0.2)
    assert got[2] == want[2] == count and got[5] == want[5] == count
    for k in (0, 1, 3, 4):
        assert got[k] == pytest.approx(want[k], rel=1e-5)
    dim1, dim2 = grid_mesh(*got)
    assert dim1.shape == dim2.shape == (count, count) and dim1.dtype == np.float32
    assert dim1[0, 0] == np.float32(got[0]) and dim2[0, 0] == np.float32(got[3])
    hi0 = float(x[:, 0].max()) + 0.1 * float(x[:, 0].max() - x[:, 0].min())
    assert dim1.max() < hi0 <= dim1.max() + got[1] * (1 + 1e-5)        # tf.range stops before the limit, within a step of it


def test_grid_rows_are_in_ij_order():
    a0, da, n1, b0, db, n2 = -1.0, 0.25, 3, 2.0, 0.5, 4
    rows = pc.grid_rows_f32(np.eye(2), a0, da, n1, b0, db, n2)
    dim1, dim2 = grid_mesh(a0, da, n1, b0, db, n2)
    np.testing.assert_array_equal(rows, np.stack([dim1.reshape(-1), dim2.reshape(-1)], axis=1))
    assert rows[1].tolist() == [-1.0, 2.5] and rows[n2].tolist() == [-0.75, 2.0]      # the second axis runs fastest
    np.testing.assert_array_equal(pc.grid_rows_f32(np.eye(2), a0, da, n1, b0, db, n2, 5, 4), rows[5:9])


# ---------------------------------------------------------------- PCA
def test_pca_axes_against_svd_and_sklearn():
    rng = np.random.default_rng(13)
    x = rng.normal(size=(50, 5)) @ rng.normal(size=(5, 5)) + rng.normal(size=5)
    axes = pca_axes(x, 2)
    _, _, vt = np.linalg.svd(x - x.mean(axis=0), full_matrices=False)
    assert axes.shape == (5, 2) and axes.dtype == np.float64
    for k in range(2):
        assert np.allclose(axes[:, k], vt[k], atol=1e-12) or np.allclose(axes[:, k], -vt[k], atol=1e-12)
        assert axes[np.argmax(np.abs(axes[:, k])), k] > 0           # the sign rule
    np.testing.assert_allclose(axes.T @ axes, np.eye(2), atol=1e-12)
    np.testing.assert_array_equal(pca_axes(-x, 2), axes)            # a property of the data's spread, not of its sign
    with pytest.raises(ValueError):
        pca_axes(x[:, :1], 2)
    decomposition = pytest.importorskip("sklearn.decomposition")
    for k in (2, 3):
        sk = decomposition.PCA(n_components=k, svd_solver="full").fit(x)
        mine, t = pca_axes(x, k), pca_transform(x, k)
        ref_t = sk.transform(x)
        for c in range(k):
            sign = np.sign(mine[:, c] @ sk.components_[c])
            np.testing.assert_allclose(mine[:, c], sign * sk.components_[c], atol=1e-10)
            np.testing.assert_allclose(t[:, c], sign * ref_t[:, c], atol=1e-10)


# ---------------------------------------------------------------- ROC and confusion matrix
def _scores():
    rng = np.random.default_rng(14)
    y = rng.integers(0, 3, size=120)
    p = rng.dirichlet(np.ones(3), size=120)
    p[np.arange(120), y] += 0.3
    p = np.round(p / p.sum(axis=1, keepdims=True), 2)                 # ties between scores
    return y, p


def test_roc_curve_against_sklearn_and_the_micro_auroc():
    y, p = _scores()
    for label in range(3):
        fpr, tpr, thr = roc_curve(y == label, p[:, label])
        assert fpr[0] == tpr[0] == 0.0 and fpr[-1] == tpr[-1] == 1.0 and thr[0] == np.inf
        assert (np.diff(fpr) >= 0).all() and (np.diff(tpr) >= 0).all() and (np.diff(thr) < 0).all()
        assert len(thr) == len(np.unique(p[:, label])) + 1          # every distinct score is a threshold
        area = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))
        # Metrics.micro_auroc of ONE column takes label 0 as the positive class: the indicator goes in as 0
        assert area == pytest.approx(micro_auroc(np.where(y == label, 0, 1), p[:, label:label + 1]), rel=1e-12)
    metrics = pytest.importorskip("sklearn.metrics")
    for label in range(3):
        fpr, tpr, thr = roc_curve(y == label, p[:, label])
        f, t, h = metrics.roc_curve(y == label, p[:, label], drop_intermediate=False)
        np.testing.assert_allclose(fpr, f, rtol=0, atol=1e-15)
        np.testing.assert_allclose(tpr, t, rtol=0, atol=1e-15)
        np.testing.assert_array_equal(thr[1:], h[1:])


def test_confusion_counts_of_a_hand_made_case_with_an_empty_row():
    labels, counts, norm = confusion_counts([0, 0, 1, 3, 3, 3], [0, 2, 1, 1, 3, 0])
    assert labels.tolist() == [0, 1, 2, 3]                          # the union: 2 is only ever predicted
    assert counts.tolist() == [[1, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 1]]
    assert norm.tolist() == [[0.5, 0.0, 0.5, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.33, 0.33, 0.0, 0.33]]


# ---------------------------------------------------------------- the class over a stubbed model
class _Data:
    def __init__(self, x, y, regression=False):
        self.likelihood_model = "Regression" if regression else "Classification"
        n = len(x)
        self.train_data = ArrayDataset(x[:n // 2], y[:n // 2])
        self.test_data = ArrayDataset(x[n // 2:3 * n // 4], y[n // 2:3 * n // 4])
        self.valid_data = ArrayDataset(x[3 * n // 4:], y[3 * n // 4:])


class _Stub:
    """A model whose mean prediction is a fixed function of the input row, and that records its calls."""

    def __init__(self, d=2, C=3):
        self.calls = []
        self.W = np.random.default_rng(15).normal(size=(d, C))

    def _mean(self, x):
        z = np.asarray(x, dtype=np.float64).reshape(len(x), -1) @ self.W
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)

    def _summary(self, mean):
        top, cls, _, _ = pc.summary(mean)
        return mean, top, cls.astype(np.int32), pc.entropy_f32(mean)

    def predictive_surface(self, x, nb_samples, column=0, want_cols=False):
        self.calls.append(("predictive_surface", len(x), nb_samples))
        return (None,) + self._summary(self._mean(x))

    def grid_surface(self, basis, a0, da, n1, b0, db, n2, nb_samples, column=0, want_cols=False):
        self.calls.append(("grid_surface", np.asarray(basis), (a0, da, n1, b0, db, n2), nb_samples, column, want_cols))
        rows = pc.grid_rows_f32(basis, a0, da, n1, b0, db, n2)
        # the "column of a draw" is a code of the grid point: the tests read the row order off it
        cols = np.repeat((rows[:, 0] + np.float32(100.0) * rows[:, 1])[None], nb_samples, axis=0) if want_cols else None
        return (cols,) + self._summary(self._mean(rows))

    def predict(self, x, nb_samples):
        self.calls.append(("predict", len(x), nb_samples))
        x = np.asarray(x, dtype=np.float32).reshape(len(x), -1)
        samples = np.stack([2.0 * x[:, :1] + 0.1 * s * np.sin(x[:, :1]) for s in range(nb_samples)]).astype(np.float32)
        return list(samples), samples.mean(axis=0)


def _classification(d=2, n=80):
    rng = np.random.default_rng(16)
    x = rng.normal(size=(n, d)).astype(np.float32)
    stub = _Stub(d)
    y = stub._mean(x).argmax(axis=1).astype(np.int32)
    y[::5] = (y[::5] + 1) % 3
    data = _Data(x, y)
    return stub, data, Plotter(stub, data)


def _regression(y_shape=(80, 1)):
    rng = np.random.default_rng(17)
    x = rng.uniform(-2, 2, size=(80, 1)).astype(np.float32)
    y = (2.0 * x + 0.2 * rng.normal(size=x.shape)).astype(np.float32).reshape(y_shape)
    stub = _Stub(1)
    data = _Data(x, y, regression=True)
    return stub, data, Plotter((stub, None), data)


def test_get_x_y_takes_the_first_rows_of_the_named_split():
    _, data, pl = _classification()
    for data_type, split in (("test", data.test_data), ("train", data.train_data), ("valid", data.valid_data),
                             ("anything", data.valid_data)):
        x, y = pl._get_x_y(7, data_type)
        np.testing.assert_array_equal(x, split.x[:7])
        np.testing.assert_array_equal(y, split.y[:7])
    assert len(pl._get_x_y(1000, "test")[0]) == 20


def test_decision_boundaries_always_draw_ten_and_keep_the_row_order():
    stub, data, pl = _classification()
    d = pl.decision_boundaries_data(granularity=0.21, n_boundaries=3, n_samples=15, data_type="train")
    (name, basis, grid, draws, column, want_cols), = stub.calls
    assert name == "grid_surface" and draws == 10 and column == 0 and want_cols is True      # :191-192: ten, not three
    np.testing.assert_array_equal(basis, np.eye(2, dtype=np.float32))
    assert grid == grid_axes(data.train_data.x[:15], 0.21, 0.2) and grid[2] == grid[5] == 5
    assert d["boundaries"].shape == (10, 5, 5) and d["n_boundaries"] == 10
    np.testing.assert_array_equal(d["boundaries"][7], d["dim1"] + np.float32(100.0) * d["dim2"])
    np.testing.assert_array_equal(d["x"], data.train_data.x[:15])
    np.testing.assert_array_equal(d["y"], data.train_data.y[:15])


def test_uncertainty_area_uses_n_samples_as_draws_and_masks_below_the_threshold():
    stub, data, pl = _classification()
    d = pl.uncertainty_area_data(granularity=0.13, n_samples=17, uncertainty_threshold=0.6)
    (name, basis, grid, draws, column, want_cols), = stub.calls
    assert name == "grid_surface" and draws == 17 and want_cols is False                     # :63
    assert d["top"].shape == (8, 8)
    np.testing.assert_array_equal(d["uncertain"], (d["top"] < np.float32(0.6)).astype(np.float32))
    assert 0 < d["uncertain"].sum() < 64
    np.testing.assert_array_equal(d["classes"], np.unique(data.test_data.y[:17]))
    stub3, _, pl3 = _classification(d=3)                                                     # nothing for dimension != 2
    assert pl3.uncertainty_area_data(dimension=3) is None and pl3.plot_uncertainty_area(dimension=3) is None
    assert stub3.calls == []


def test_wider_inputs_go_through_the_pca_basis(capsys):
    stub, data, pl = _classification(d=5)
    d = pl.uncertainty_area_data(granularity=0.3, n_samples=20)
    assert "Will apply PCA to reduce to dimension  2" in capsys.readouterr().out
    x = data.test_data.x[:20]
    base = pca_axes(x, 2).astype(np.float32)
    np.testing.assert_array_equal(d["base_matrix"], base)
    np.testing.assert_array_equal(stub.calls[0][1], base)
    np.testing.assert_array_equal(d["x"], x @ base)
    assert stub.calls[0][2] == grid_axes(x @ base, 0.3, 0.2) and d["top"].shape == (4, 4)


def test_entropy_is_nan_to_numd_then_sorted():
    stub, data, pl = _classification()
    real = stub.predictive_surface

    def with_nan(*a, **k):
        out = list(real(*a, **k))
        out[4] = out[4].copy()
        out[4][3], out[4][5] = np.nan, np.inf
        return tuple(out)

    stub.predictive_surface = with_nan
    ent = pl.entropy_data(n_boundaries=4, n_samples=20)
    raw = real(data.test_data.x[:20], 4)[4].copy()
    raw[3], raw[5] = 0.0, np.finfo(np.float32).max
    np.testing.assert_array_equal(ent, np.sort(raw))
    assert ent[-1] == np.finfo(np.float32).max and (np.diff(ent) >= 0).all() and np.isfinite(ent).all()


def test_classification_data_methods_read_the_surface_once():
    stub, data, pl = _classification()
    x, y = data.test_data.x, data.test_data.y
    mean, _, cls, _ = stub._summary(stub._mean(x))
    labels, counts, norm = pl.confusion_matrix_data(n_boundaries=6, n_samples=20)
    ref = confusion_counts(y, cls)
    assert labels.tolist() == ref[0].tolist() and counts.tolist() == ref[1].tolist() and norm.tolist() == ref[2].tolist()
    fpr, tpr, thr = pl.roc_data(n_samples=20, label_of_interest=2, n_boundaries=6)
    ref = roc_curve(y == 2, mean[:, 2])
    for a, b in zip((fpr, tpr, thr), ref):
        np.testing.assert_array_equal(a, b)
    cmp = pl.compare_prediction_to_target_data(n_boundaries=6, n_samples=20)
    assert cmp["kind"] == "2d" and cmp["y_pred"].tolist() == cls.tolist() and cmp["y_true"].tolist() == y.tolist()
    np.testing.assert_array_equal(cmp["x"], x)
    assert stub.calls == [("predictive_surface", 20, 6)]                                      # one read-out for the three


def test_the_cache_is_keyed_by_draws_target_shape_and_split():
    stub, data, pl = _classification()
    pl.entropy_data(n_boundaries=6, n_samples=20)
    pl.entropy_data(n_boundaries=6, n_samples=20)
    assert len(stub.calls) == 1
    pl.entropy_data(n_boundaries=7, n_samples=20)
    assert len(stub.calls) == 2
    pl.entropy_data(n_boundaries=7, n_samples=12)                   # another shape of y_true
    assert stub.calls[-1] == ("predictive_surface", 12, 7) and len(stub.calls) == 3
    pl.entropy_data(n_boundaries=7, n_samples=12, data_type="valid")
    assert len(stub.calls) == 4
    pl.entropy_data(n_boundaries=7, n_samples=12, data_type="valid")
    assert len(stub.calls) == 4
    pl.entropy_data(n_boundaries=6, n_samples=20)                   # one entry is kept, as in the reference
    assert len(stub.calls) == 5


def test_compare_prediction_to_target_projects_wider_inputs():
    stub, data, pl = _classification(d=5)
    cmp = pl.compare_prediction_to_target_data(n_samples=20)
    assert cmp["kind"] == "3d" and cmp["x"].shape == (20, 3)
    np.testing.assert_array_equal(cmp["x"], pca_transform(data.test_data.x, 3))
    stub, data, pl = _regression()
    cmp = pl.compare_prediction_to_target_data(n_boundaries=5, n_samples=20)
    assert cmp["kind"] == "regression" and cmp["y_true"].shape == cmp["y_pred"].shape == (20, 1)
    assert stub.calls == [("predict", 20, 5)]


@pytest.mark.parametrize("y_shape", [(80, 1), (80,)], ids=str)
def test_regression_uncertainty_is_the_reference_arithmetic(y_shape):
    stub, data, pl = _regression(y_shape)
    pred_dev, err = pl.regression_uncertainty_data(n_boundaries=5, n_samples=20)
    y_samples, y_pred = _Stub(1).predict(data.test_data.x, 5)
    y_true = data.test_data.y
    variance = np.var(np.asarray(y_samples, dtype=np.float64), axis=0)
    np.testing.assert_array_equal(err, np.mean(np.sqrt(variance), axis=1))
    np.testing.assert_array_equal(pred_dev, np.mean((y_pred - y_true), axis=1))
    assert err.shape == pred_dev.shape == (20,) and (err > 0).any()
    # float64: the spread of draws that differ in the eighth digit is not lost
    assert np.var(np.float64(1.0) + np.arange(3) * 1e-9) > 0


def test_every_exception_of_the_reference():
    stub, data, pl = _classification()
    with pytest.raises(ValueError, match="regression uncertainty cannot be computed for other than regression problems"):
        pl.regression_uncertainty()
    stub3, _, pl3 = _classification(d=3)
    with pytest.raises(ValueError, match="Decision boundary can only be plotted in 2 dimensions"):
        pl3.plot_decision_boundaries(dimension=3)
    assert stub3.calls == []
    with pytest.raises(ValueError, match="is inferior to given dimension"):
        pl.plot_decision_boundaries(dimension=3)
    with pytest.raises(ValueError, match="is inferior to given dimension"):
        pl.plot_uncertainty_area(dimension=3)
    assert stub.calls == []
    stub, data, pl = _regression()
    for method, message in ((pl.roc_one_vs_rest, "ROC can only be plotted for Classification"),
                            (pl.plot_decision_boundaries, "Decision boundary can only be plotted for Classification"),
                            (pl.plot_uncertainty_area, "Uncertainty area can only be plotted for Classification"),
                            (pl.confusion_matrix, "Confusion matrix cannot be computed for other than classification problems")):
        with pytest.raises(ValueError, match=message):
            method()
    with pytest.raises(Exception, match="Entropy is only available for classification") as info:
        pl.entropy()
    assert info.type is Exception
    assert stub.calls == []


def test_signatures_and_defaults_are_the_reference_s():
    import inspect
    want = {"roc_one_vs_rest": dict(n_samples=100, label_of_interest=0, n_boundaries=10, data_type="test"),
            "plot_decision_boundaries": dict(dimension=2, granularity=1e-2, n_boundaries=30, n_samples=100, data_type="test",
                                             un_zoom_level=0.2, save_path=None),
            "plot_uncertainty_area": dict(dimension=2, granularity=1e-2, n_samples=100, data_type="test",
                                          uncertainty_threshold=0.8, un_zoom_level=0.2, save_path=None),
            "regression_uncertainty": dict(n_boundaries=30, n_samples=100, data_type="test", save_path=None),
            "confusion_matrix": dict(n_boundaries=30, n_samples=100, data_type="test", save_path=None),
            "compare_prediction_to_target": dict(n_boundaries=30, n_samples=100, data_type="test", save_path=None),
            "entropy": dict(n_boundaries=30, n_samples=100, data_type="test", save_path=None)}
    for name, params in want.items():
        sig = inspect.signature(getattr(Plotter, name)).parameters
        got = {k: v.default for k, v in sig.items() if k != "self"}
        assert list(got)[:len(params)] == list(params) and {k: got[k] for k in params} == params, name
    assert list(inspect.signature(Plotter.learning_diagnostics).parameters) == ["self", "loss_file", "save_path"]
    for name in ("decision_boundaries_data", "uncertainty_area_data", "roc_data", "confusion_matrix_data", "entropy_data",
                 "regression_uncertainty_data", "compare_prediction_to_target_data"):
        assert callable(getattr(Plotter, name))


def test_every_plotting_method_writes_its_png(tmp_path):
    pytest.importorskip("matplotlib")
    path = str(tmp_path)
    stub, data, pl = _classification()
    pl.plot_decision_boundaries(granularity=0.13, n_samples=20, save_path=path)
    pl.plot_uncertainty_area(granularity=0.13, n_samples=20, uncertainty_threshold=0.6, save_path=path)
    pl.confusion_matrix(n_samples=20, save_path=path)
    pl.entropy(n_samples=20, save_path=path)
    pl.roc_one_vs_rest(n_samples=20, save_path=path)
    pl.compare_prediction_to_target(n_samples=20, save_path=path)
    plots = tmp_path / "report" / "plots"
    for name in ("decision_boundaries", "uncertainty_area", "confusion_matrix", "entropy", "roc_one_vs_rest",
                 "comparison_pred_true"):
        assert (plots / (name + ".png")).stat().st_size > 0, name
    (plots / "comparison_pred_true.png").unlink()
    _classification(d=5)[2].compare_prediction_to_target(n_samples=20, save_path=path)      # the 3-D scatter
    assert (plots / "comparison_pred_true.png").stat().st_size > 0
    (plots / "comparison_pred_true.png").unlink()
    stub, data, pl = _regression()
    pl.regression_uncertainty(n_boundaries=5, n_samples=20, save_path=path)
    pl.compare_prediction_to_target(n_boundaries=5, n_samples=20, save_path=path)
    losses = tmp_path / "losses.txt"
    losses.write_text("\n".join(str(1.0 / (k + 1)) for k in range(30)))
    pl.learning_diagnostics(str(losses), save_path=path)
    assert pl.learning_diagnostics(None, save_path=path) is None
    for name in ("epistemic_uncertainty", "comparison_pred_true", "learning_diagnostics"):
        assert (plots / (name + ".png")).stat().st_size > 0, name


def test_the_compat_package_hands_out_the_library_classes(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "compat"))
    for name in [n for n in sys.modules if n == "Pyesian" or n.startswith("Pyesian.")]:
        monkeypatch.delitem(sys.modules, name)
    import Pyesian.visualisations as cv
    assert cv.Plotter is Plotter and cv.Metrics is Metrics
    src = open(os.path.join(ROOT, "compat", "Pyesian", "visualisations", "__init__.py")).read()
    assert "class " not in src and "def " not in src               # re-exports only
    for name in [n for n in sys.modules if n == "Pyesian" or n.startswith("Pyesian.")]:
        sys.modules.pop(name, None)


def test_the_entropy_bound_holds_for_numpy_float32():
    """The bound of the device test is derived, not measured; NumPy's float32 arithmetic of the same sum stays under it."""
    rng = np.random.default_rng(18)
    for C_out in (1, 2, 3, 10, 300):
        mean = rng.dirichlet(np.full(max(C_out, 2), 0.3), size=1600).astype(np.float32)[:, :C_out]
        _, _, ent64, bound = pc.summary(mean)
        ratio = np.abs(pc.entropy_f32(mean).astype(np.float64) - ent64) / bound
        assert ratio.max() < 1.0, (C_out, ratio.max())
