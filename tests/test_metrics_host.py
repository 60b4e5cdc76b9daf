"""CPU checks of the predictive-moments entry point and of visualisations.Metrics: the C-ABI row, the closed forms of
classification_uncertainty against the reference's loop taken literally (tests/metrics_checks.py), every sklearn-derived
formula against sklearn itself, the calibration error against a hand-worked table, the reach of the device tests' case
table, and the host logic of the class over a fake model."""

import json
import math
import os
import re
import warnings

import numpy as np
import pytest

from metrics_checks import CASES, moments, surface_classification, surface_regression, uncertainty_loop
from oracle import mlp as o_mlp

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.visualisations import Metrics
from bayesian_inference_for_nn_amd.visualisations.Metrics import (accuracy_score, expected_calibration_error,
                                                                  gaussian_log_likelihood, macro_f1, macro_recall,
                                                                  mean_absolute_error, mean_squared_error, micro_auroc,
                                                                  micro_precision, r2_score, root_mean_squared_error,
                                                                  two_columns, uncertainty_from_moments)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"pyz_mlp *": _lib._p, "const float *": _lib._p, "float *": _lib._p, "void *": _lib._p, "int": _lib.C.c_int}


# ---------------------------------------------------------------- the entry point
def test_entry_point_is_declared_with_matching_argument_types():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pyz.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+pyz_predict_moments\s*\(([^)]*)\)\s*;", src)
    assert proto, "pyz_predict_moments is not declared in include/pyz.h"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    types = [re.sub(r"\s*\w+$", "", p) if "*" not in p else p[:p.rindex("*")].strip() + " *" for p in params]
    restype, argtypes = _lib.SIGNATURES["pyz_predict_moments"]
    assert restype is _lib.C.c_int
    assert [CTYPE[t] for t in types] == list(argtypes) and len(argtypes) == 8
    assert hasattr(_lib.load(), "pyz_predict_moments")
    assert _lib.header_version() == 302


def test_null_plan_is_refused_without_a_gpu():
    lib = _lib.load()
    rc = lib.pyz_predict_moments(None, None, 1, None, 1, None, None, None)
    assert rc < 0 and b"null plan" in lib.pyz_last_error()


def test_case_table_reaches_what_the_issue_lists():
    assert {c.C for c in CASES} == {1, 2, 3, 10, 33}
    assert {c.n for c in CASES} == {1, 5, 64, 257}
    assert {c.draws for c in CASES} == {1, 2, 7, 33}
    for C in (1, 2, 3, 10, 33):
        mine = [c for c in CASES if c.C == C]
        assert {c.n for c in mine} == {1, 5, 64, 257} and {c.softmax for c in mine} == {True, False}
        assert {c.chunks for c in mine} >= {1, 2, 3}
    for draws in (7, 33):       # one chunk, two and three chunks with a ragged last one
        mine = [c for c in CASES if c.draws == draws]
        assert {c.chunks for c in mine} == {1, 2, 3}
        assert any(c.draws % c.max_p for c in mine if c.chunks == 2) and any(c.draws % c.max_p for c in mine if c.chunks == 3)
    assert {c.chunks for c in CASES if c.draws == 2} == {1, 2}
    assert any(c.nan_draw >= 0 and c.softmax for c in CASES) and any(c.nan_draw >= 0 and not c.softmax for c in CASES)
    assert len(CASES) <= 40


def test_surface_data_keep_float32_away_from_every_decision():
    """tests/test_gpu_metrics.py compares counts, ranks and bins of the device's float32 mean with the float64 forward's
    exactly: the data must leave every argmax, every pair of distinct scores and every calibration bin edge a margin
    (>= 1e-5) that float32 forward passes of this size (errors of a few 1e-7) cannot cross."""
    s = surface_classification()
    x, y = s.dataset.test_data.as_numpy()
    assert len(x) == 60 and set(np.unique(y)) == {0, 1}
    p = o_mlp.predict(s.thetas[0], x, s.spec)
    assert np.abs(p[:, 0] - p[:, 1]).min() > 0.2
    assert 50.0 < 100.0 * (p.argmax(axis=1) == y).mean() < 100.0
    flat = np.sort(p.reshape(-1))
    assert np.diff(flat).min() > 1e-5, "two scores too close for a float32 rank"
    e = np.exp(p - p.max(axis=1, keepdims=True))
    conf = (e / e.sum(axis=1, keepdims=True)).max(axis=1)
    for n_bins in (5, 3):
        assert np.abs(conf * n_bins - np.round(conf * n_bins)).min() > 1e-4
        assert len(np.unique(np.floor(conf * n_bins))) >= 2          # more than one bin in use
    several = surface_classification(k=4)
    assert several.thetas.shape[0] == 4 and len(several.dataset.test_data) == 60
    r = surface_regression()
    xr, yr = r.dataset.test_data.as_numpy()
    assert len(xr) == 50 and 0.5 < r2_score(yr, o_mlp.predict(r.thetas[0], xr, r.spec)) < 1.0


# ---------------------------------------------------------------- classification_uncertainty: closed form == the loop
def _probabilities(rng, S, rows, C):
    if C == 1:
        return rng.uniform(0.0, 1.0, size=(S, rows, 1))
    z = rng.normal(size=(S, rows, C)) * 2.0
    e = np.exp(z - z.max(axis=2, keepdims=True))
    return e / e.sum(axis=2, keepdims=True)


@pytest.mark.parametrize("C", [1, 2, 3, 10])
@pytest.mark.parametrize("S,rows,n_samples", [(1, 1, 1), (5, 7, 7), (4, 6, 100)])
def test_closed_forms_equal_the_literal_loop(C, S, rows, n_samples):
    rng = np.random.default_rng(10 * C + S)
    p = _probabilities(rng, S, rows, C)
    labels = rng.integers(0, max(C, 2), size=rows)
    want = uncertainty_loop(p, labels, n_samples)
    mean, m2, _ = moments(p)
    got = uncertainty_from_moments(mean, m2, S, n_samples)
    for g, w, what in zip(got, want, ("total", "aleatoric", "epistemic")):
        assert g.shape == w.shape == (rows, max(C, 2), max(C, 2)) and g.dtype == np.float64
        diff = np.abs(g - w).max()
        print(f"{what}: max |closed form - loop| = {diff:.3e}, max |loop| = {np.abs(w).max():.3e}")
        assert diff <= 1e-12 * max(1.0, np.abs(w).max())
    np.testing.assert_allclose(got[0], got[1] + got[2], rtol=0, atol=1e-12)
    # the label drops out of the loop: other labels, the same matrices
    other = uncertainty_loop(p, (labels + 1) % max(C, 2), n_samples)
    assert np.abs(other[2] - want[2]).max() <= 1e-12 * max(1.0, np.abs(want[2]).max())


def test_one_output_moments_become_two_columns():
    rng = np.random.default_rng(5)
    p = rng.uniform(size=(6, 4, 1))
    mean, m2, _ = moments(p)
    q = np.concatenate([1.0 - p, p], axis=2)
    qmean, qm2, _ = moments(q)
    got_mean, got_m2 = two_columns(mean, m2, 6)
    np.testing.assert_allclose(got_mean, qmean, rtol=0, atol=1e-14)
    np.testing.assert_allclose(got_m2, qm2, rtol=0, atol=1e-13)


# ---------------------------------------------------------------- the sklearn-derived formulas against sklearn
def _label_cases():
    rng = np.random.default_rng(11)
    t = rng.integers(0, 4, size=200)
    p = np.where(rng.uniform(size=200) < 0.6, t, rng.integers(0, 4, size=200))
    yield "random", t, p
    yield "class absent from the predictions", np.array([0, 1, 2, 2, 1, 0, 2]), np.array([0, 1, 1, 0, 1, 0, 1])
    yield "class absent from the truth", np.array([0, 1, 1, 0, 1, 0, 1]), np.array([0, 1, 2, 2, 1, 0, 2])
    yield "disjoint", np.array([0, 0, 0]), np.array([1, 1, 2])
    yield "binary", np.array([0, 1, 1, 0]), np.array([1, 1, 0, 0])


@pytest.mark.parametrize("name,t,p", list(_label_cases()), ids=[c[0] for c in _label_cases()])
def test_label_metrics_equal_sklearn(name, t, p):
    skmet = pytest.importorskip("sklearn.metrics")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # sklearn warns where a term is undefined and then counts it as 0
        want = {"accuracy": skmet.accuracy_score(t, p), "macro recall": skmet.recall_score(t, p, average="macro"),
                "micro precision": skmet.precision_score(t, p, average="micro"), "macro f1": skmet.f1_score(t, p, average="macro")}
    got = {"accuracy": accuracy_score(t, p), "macro recall": macro_recall(t, p), "micro precision": micro_precision(t, p),
           "macro f1": macro_f1(t, p)}
    for k in want:
        print(k, got[k], want[k])
        assert abs(got[k] - want[k]) <= 1e-12, k


def _score_cases():
    rng = np.random.default_rng(12)
    t = rng.integers(0, 3, size=150)
    s = rng.uniform(size=(150, 3))
    s[np.arange(150), t] += 0.4
    yield "random", t, s / s.sum(axis=1, keepdims=True)
    yield "tied scores", np.array([0, 1, 1, 0, 1, 2]), np.array([[.5, .25, .25], [.5, .25, .25], [.25, .5, .25], [.25, .5, .25],
                                                                  [.25, .25, .5], [1 / 3, 1 / 3, 1 / 3]])
    yield "all tied", np.array([0, 1, 0]), np.full((3, 2), 0.5)
    yield "two columns", np.array([0, 1, 1, 0, 1]), np.array([[.9, .1], [.2, .8], [.6, .4], [.6, .4], [.5, .5]])


@pytest.mark.parametrize("name,t,s", list(_score_cases()), ids=[c[0] for c in _score_cases()])
def test_auroc_equals_sklearn(name, t, s):
    skmet = pytest.importorskip("sklearn.metrics")
    hot = (t[:, None] == np.arange(s.shape[1])[None, :]).astype(np.float64)
    want = skmet.roc_auc_score(hot, s, average="micro", multi_class="ovr")
    got = micro_auroc(t, s)
    print(got, want)
    assert abs(got - want) <= 1e-12


def _regression_cases():
    rng = np.random.default_rng(13)
    y = rng.normal(size=(80, 1))
    yield "random", y, y + 0.3 * rng.normal(size=y.shape)
    y2 = rng.normal(size=(60, 2)) * np.array([1.0, 5.0])
    yield "two output columns", y2, y2 + rng.normal(size=y2.shape) * np.array([0.1, 2.0])
    const = np.stack([np.full(30, 2.5), rng.normal(size=30)], axis=1)
    yield "constant target column", const, const + 0.2 * rng.normal(size=const.shape)
    exact = np.stack([np.full(30, 2.5), rng.normal(size=30)], axis=1)
    pred = exact.copy()
    pred[:, 1] += 0.1
    yield "constant target column predicted exactly", exact, pred
    yield "flat target, (rows,) against (rows, 1)", rng.normal(size=40), rng.normal(size=(40, 1))


@pytest.mark.parametrize("name,y,p", list(_regression_cases()), ids=[c[0] for c in _regression_cases()])
def test_regression_metrics_equal_sklearn(name, y, p):
    skmet = pytest.importorskip("sklearn.metrics")
    want = {"mse": skmet.mean_squared_error(y, p), "rmse": skmet.root_mean_squared_error(y, p),
            "mae": skmet.mean_absolute_error(y, p), "r2": skmet.r2_score(y, p)}
    got = {"mse": mean_squared_error(y, p), "rmse": root_mean_squared_error(y, p), "mae": mean_absolute_error(y, p),
           "r2": r2_score(y, p)}
    for k in want:
        print(k, got[k], want[k])
        assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), k
    yy, pp = np.asarray(y, dtype=np.float64).reshape(len(p), -1), np.asarray(p).reshape(len(p), -1)
    ll = np.mean([-0.5 * (a - b) ** 2 - 0.5 * math.log(2 * math.pi) for a, b in zip(pp.ravel(), yy.ravel())])
    assert abs(gaussian_log_likelihood(y, p) - ll) <= 1e-12


# ---------------------------------------------------------------- the calibration error against a worked table
def test_ece_equals_the_hand_worked_table():
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "metrics_ece_table.json")))
    logits, labels, n_bins = np.array(table["logits"]), np.array(table["labels"]), table["n_bins"]
    # the table itself: its per-bin lines add up to its total, a confidence sits on a bin edge, a bin is empty
    assert table["rows_on_a_bin_edge"] and any(b["count"] == 0 for b in table["bins"])
    total = sum(b["count"] / len(labels) * abs(b["accuracy"] - b["confidence"]) for b in table["bins"] if b["count"])
    assert abs(total - table["ece"]) <= 1e-15
    got = expected_calibration_error(n_bins, logits, labels)
    print(got, table["ece"])
    assert abs(got - table["ece"]) <= 1e-12
    # one-row sub-tables: the bin each row lands in
    for row, want_bin, conf in zip(range(len(labels)), table["row_bin"], table["row_confidence"]):
        e = np.exp(logits[row] - logits[row].max())
        assert (e / e.sum()).max() == conf
        assert int(np.clip(np.floor(conf * n_bins), 0, n_bins - 1)) == want_bin


# ---------------------------------------------------------------- the class over a fake model
class _Split:
    def __init__(self, x, y):
        self.x, self.y = np.asarray(x), np.asarray(y)

    def batch(self, n):
        return iter([(self.x[:n], self.y[:n])])


class _Data:
    def __init__(self, kind, test, train, valid):
        self.likelihood_model = kind
        self.test_data, self.train_data, self.valid_data = _Split(*test), _Split(*train), _Split(*valid)


class _Model:
    """predictive_moments / predictive_mean of a fixed table keyed by the first input column; counts its calls."""

    def __init__(self, C, draws_seed=0):
        self.C, self.calls, self.seed = C, [], draws_seed

    def _samples(self, x, nb):
        rng = np.random.default_rng(self.seed + nb)
        base = rng.normal(size=(nb, 1, self.C)) * 0.3 + np.asarray(x, dtype=np.float64)[None, :, :1] * np.arange(1, self.C + 1)
        if self.C == 1:
            return 1.0 / (1.0 + np.exp(-base))
        e = np.exp(base - base.max(axis=2, keepdims=True))
        return e / e.sum(axis=2, keepdims=True)

    def predictive_moments(self, x, nb):
        self.calls.append(("moments", len(x), nb))
        mean, m2, _ = moments(self._samples(x, nb))
        return mean.astype(np.float32), m2.astype(np.float32), nb

    def predictive_mean(self, x, nb):
        self.calls.append(("mean", len(x), nb))
        return (np.asarray(x, dtype=np.float64)[:, :1] * np.arange(1, self.C + 1)).astype(np.float32)

    def predict(self, *a, **k):
        raise AssertionError("Metrics must not fetch the sample tensor")


def _classification_data(rows=12, C=3):
    rng = np.random.default_rng(3)
    mk = lambda n, s: (rng.normal(size=(n, 2)) + s, rng.integers(0, max(C, 2), size=n))
    return _Data("Classification", mk(rows, 0.0), mk(rows, 1.0), mk(rows, 2.0))


def test_classification_methods_print_save_and_cache(capsys, tmp_path):
    data, model = _classification_data(), _Model(3)
    m = Metrics((model, "ignored"), data)                       # an optimizer's result() tuple
    out = m.summary(n_boundaries=5, n_samples=8, save_path=str(tmp_path))
    assert list(out) == ["accuracy", "recall", "precision", "f1_score", "auroc", "ece"]
    assert model.calls == [("moments", 8, 5)]                   # one read-out for the six metrics
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"Accuracy: {out['accuracy']}%", f"Recall: {out['recall']}%", f"Precision: {out['precision']}%",
                     f"F1 score: {out['f1_score']}", f"AUROC: {out['auroc']}", f"ECE: {out['ece']}"]
    for name, key in (("Accuracy", "accuracy"), ("Recall", "recall"), ("Precision", "precision"), ("F1_score", "f1_score"),
                      ("AUROC", "auroc"), ("ECE", "ece")):
        assert (tmp_path / "report" / name).read_text() == str(out[key])
    # the values: the host formulas on the model's mean
    x, y = data.test_data.x[:8], data.test_data.y[:8]
    mean = moments(model._samples(x, 5))[0].astype(np.float32).astype(np.float64)
    pred = mean.argmax(axis=1)
    assert out["accuracy"] == accuracy_score(y, pred) * 100 and out["precision"] == macro_recall(y, pred) * 100
    assert out["recall"] == micro_precision(y, pred) * 100 and out["f1_score"] == macro_f1(y, pred)
    assert out["auroc"] == micro_auroc(y, mean) and out["ece"] == expected_calibration_error(5, mean, y)
    assert m.ece(n_boundaries=5, n_samples=8, n_bins=3) == expected_calibration_error(3, mean, y)
    # uncertainty: the closed form of the same cached read-out, equal to the loop on the model's samples
    total, alea, epi = m.classification_uncertainty(n_boundaries=5, n_samples=8)
    assert model.calls == [("moments", 8, 5)]
    want = uncertainty_loop(model._samples(x, 5), y, 8)
    for g, w in zip((total, alea, epi), want):
        assert g.shape == (8, 3, 3) and np.abs(g - w).max() <= 1e-5            # (the fake hands float32 moments back)
    # other keys miss: draws, split (same rows: the reference would return the test split's numbers), rows
    a_test = m.accuracy(n_boundaries=5, n_samples=8)
    m.accuracy(n_boundaries=6, n_samples=8)
    a_train = m.accuracy(n_boundaries=5, n_samples=8, data_type="train")
    m.accuracy(n_boundaries=5, n_samples=8, data_type="anything else")        # the validation split
    m.accuracy(n_boundaries=5, n_samples=7)
    assert model.calls[1:] == [("moments", 8, 6), ("moments", 8, 5), ("moments", 8, 5), ("moments", 7, 5)]
    yt = data.train_data.y[:8]
    mt = moments(model._samples(data.train_data.x[:8], 5))[0].astype(np.float32).astype(np.float64)
    assert a_train == accuracy_score(yt, mt.argmax(axis=1)) * 100 and a_test == out["accuracy"]
    m.accuracy(n_boundaries=5, n_samples=8, data_type="train")
    assert len(model.calls) == 5                                               # a hit
    # n_samples beyond the split: the whole split
    m.accuracy(n_boundaries=5, n_samples=100)
    assert model.calls[-1] == ("moments", 12, 5)
    for name in ("mse", "rmse", "mae", "r2", "log_likeliood"):
        with pytest.raises(Exception, match="could only be computed for regression"):
            getattr(m, name)()


def test_one_output_classifier_is_read_as_two_columns(capsys):
    data, model = _classification_data(C=1), _Model(1)
    m = Metrics(model, data)
    out = m.summary(n_boundaries=4, n_samples=10)
    x, y = data.test_data.x[:10], data.test_data.y[:10]
    p = moments(model._samples(x, 4))[0].astype(np.float32).astype(np.float64)
    mean = np.concatenate([1.0 - p, p], axis=1)
    assert out["accuracy"] == accuracy_score(y, mean.argmax(axis=1)) * 100
    assert out["auroc"] == micro_auroc(y, mean) and out["ece"] == expected_calibration_error(5, mean, y)
    total, alea, epi = m.classification_uncertainty(n_boundaries=4, n_samples=10)
    want = uncertainty_loop(model._samples(x, 4), y, 10)
    assert total.shape == (10, 2, 2)
    for g, w in zip((total, alea, epi), want):
        assert np.abs(g - w).max() <= 1e-5


def test_regression_methods_print_save_and_refuse(capsys, tmp_path):
    rng = np.random.default_rng(4)
    mk = lambda n: (rng.normal(size=(n, 1)), rng.normal(size=(n, 2)))
    data, model = _Data("Regression", mk(9), mk(9), mk(9)), _Model(2)
    m = Metrics(model, data)
    out = m.summary(n_boundaries=3, n_samples=9, save_path=str(tmp_path))
    assert list(out) == ["mse", "rmse", "mae", "r2", "log_likeliood"]
    assert model.calls == [("mean", 9, 3)]
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"MSE: {out['mse']}", f"RMSE: {out['rmse']}", f"MAE: {out['mae']}", f"R2 score: {out['r2']}",
                     f"log likelihood: {out['log_likeliood']}"]
    for name, key in (("MSE", "mse"), ("RMSE", "rmse"), ("MAE", "mae"), ("R2", "r2"), ("log_likelihood", "log_likeliood")):
        assert (tmp_path / "report" / name).read_text() == str(out[key])
    y, p = data.test_data.y, model.predictive_mean(data.test_data.x, 3).astype(np.float64)
    assert out["mse"] == mean_squared_error(y, p) and out["rmse"] == root_mean_squared_error(y, p)
    assert out["mae"] == mean_absolute_error(y, p) and out["r2"] == r2_score(y, p)
    assert out["log_likeliood"] == gaussian_log_likelihood(y, p)
    for name in ("accuracy", "precision", "recall", "f1_score", "ece"):
        with pytest.raises(Exception, match="Log likelihood could only be computed for regression"):
            getattr(m, name)()
    with pytest.raises(ValueError, match="ROC can only be plotted for Classification"):
        m.auroc()
    with pytest.raises(Exception, match="only for classification"):
        m.classification_uncertainty()
    data.likelihood_model = "Ranking"
    assert m.summary() == {} and capsys.readouterr().out.endswith("Invalid loss function\n")


def test_product_package_imports_neither_sklearn_nor_tfp_nor_the_oracle():
    src = open(os.path.join(ROOT, "bayesian_inference_for_nn_amd", "visualisations", "Metrics.py")).read()
    imports = re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, flags=re.M)
    assert imports and all(i.split(".")[0] in ("__future__", "math", "os", "numpy") for i in imports), imports
    import bayesian_inference_for_nn_amd.visualisations as vis
    assert vis.Metrics is Metrics and "Metrics" in vis.__all__
