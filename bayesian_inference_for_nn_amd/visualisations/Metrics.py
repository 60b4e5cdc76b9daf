"""Performance metrics of a trained ``BayesianModel`` over a ``Dataset`` (mirrors Pyesian/visualisations/Metrics.py): the
same methods, keywords, printed lines, report files and exceptions.

Every number is NumPy float64 arithmetic on what the device hands back: the Monte-Carlo mean (rows, C) and, for
classification, the per-row second moment sum_s p_s p_s^T (rows, C, C) of the draws (``BayesianModel.predictive_moments``,
kernel pyz_predict_moments).  The (draws, rows, C) sample tensor of ``predict`` never leaves the device -- it is not even
written.  sklearn and tensorflow_probability, which the reference calls, are not imported; the functions below restate
what those calls compute, quirks of the reference's use of them included (each named where it occurs).

Deviations from the reference, on purpose:
  * the prediction cache is keyed by (n_boundaries, data_type, rows); the reference keys it by (n_boundaries, shape of
    y_true) and so returns the numbers of the split it saw first when two splits have as many rows;
  * ``summary`` returns {lowercase method name: value} (the reference returns None);
  * a one-output classifier is read as the two columns [1 - p, p] everywhere (the reference stacks them into a
    (rows, 2, 1) tensor, on which its uncertainty loop and sklearn calls fail);
  * ``log_likeliood`` pairs row i's prediction with row i's target (the reference broadcasts (rows,) targets against
    (rows, 1) predictions to rows x rows pairs).
"""

from __future__ import annotations

import math
import os

import numpy as np


# ---------------------------------------------------------------------------------------------------- regression
def _columns(y_true, y_pred):
    y_pred = np.asarray(y_pred, dtype=np.float64)
    y_pred = y_pred.reshape(len(y_pred), -1)
    y_true = np.asarray(y_true, dtype=np.float64).reshape(y_pred.shape)
    return y_true, y_pred


def mean_squared_error(y_true, y_pred) -> float:
    """sklearn's multi-output 'uniform_average': mean over the columns of mean_i (y_hat - y)^2."""
    y, p = _columns(y_true, y_pred)
    return float(((p - y) ** 2).mean(axis=0).mean())


def root_mean_squared_error(y_true, y_pred) -> float:
    """sklearn's: sqrt(mean_i (y_hat - y)^2) PER COLUMN, then the plain average of the columns."""
    y, p = _columns(y_true, y_pred)
    return float(np.sqrt(((p - y) ** 2).mean(axis=0)).mean())


def mean_absolute_error(y_true, y_pred) -> float:
    """mean over the columns of mean_i |y_hat - y|."""
    y, p = _columns(y_true, y_pred)
    return float(np.abs(p - y).mean(axis=0).mean())


def r2_score(y_true, y_pred) -> float:
    """mean over the columns of 1 - sum_i (y - y_hat)^2 / sum_i (y - mean y)^2; a column whose target is constant
    scores 1.0 when it is predicted exactly and 0.0 otherwise (sklearn's force_finite)."""
    y, p = _columns(y_true, y_pred)
    res = ((y - p) ** 2).sum(axis=0)
    tot = ((y - y.mean(axis=0)) ** 2).sum(axis=0)
    score = np.ones_like(res)
    ok = tot != 0
    score[ok] = 1.0 - res[ok] / tot[ok]
    score[~ok & (res != 0)] = 0.0
    return float(score.mean())


def gaussian_log_likelihood(y_true, y_pred) -> float:
    """mean of log N(y_hat; y, 1) = -(y_hat - y)^2 / 2 - log(2 pi) / 2 (tfp's Normal(y, 1).log_prob(y_hat))."""
    y, p = _columns(y_true, y_pred)
    return float((-0.5 * (p - y) ** 2 - 0.5 * math.log(2.0 * math.pi)).mean())


# ---------------------------------------------------------------------------------------------------- classification
def _labels(y_true, y_pred):
    y_true = np.asarray(y_true).reshape(-1).astype(np.int64)
    y_pred = np.asarray(y_pred).reshape(-1).astype(np.int64)
    return y_true, y_pred, np.union1d(y_true, y_pred)


def accuracy_score(y_true, y_pred) -> float:
    """share of rows whose predicted label is the true one."""
    t, p, _ = _labels(y_true, y_pred)
    return float((t == p).mean())


def macro_recall(y_true, y_pred) -> float:
    """sklearn's recall_score(average='macro'): mean over the UNION of true and predicted labels of tp / (tp + fn); a
    label that never occurs in y_true counts as 0."""
    t, p, labels = _labels(y_true, y_pred)
    terms = []
    for c in labels:
        tp, support = float(((t == c) & (p == c)).sum()), float((t == c).sum())
        terms.append(tp / support if support > 0 else 0.0)
    return float(np.mean(terms))


def micro_precision(y_true, y_pred) -> float:
    """sklearn's precision_score(average='micro'): sum_c tp_c / sum_c (tp_c + fp_c).  Every row is predicted as exactly
    one label, so the denominator is the row count: the accuracy."""
    t, p, labels = _labels(y_true, y_pred)
    tp = sum(float(((t == c) & (p == c)).sum()) for c in labels)
    pred = sum(float((p == c).sum()) for c in labels)
    return tp / pred if pred > 0 else 0.0


def macro_f1(y_true, y_pred) -> float:
    """sklearn's f1_score(average='macro'): mean over the union of true and predicted labels of
    2 tp / (2 tp + fp + fn) (0 where undefined)."""
    t, p, labels = _labels(y_true, y_pred)
    terms = []
    for c in labels:
        tp = float(((t == c) & (p == c)).sum())
        fp, fn = float(((t != c) & (p == c)).sum()), float(((t == c) & (p != c)).sum())
        den = 2.0 * tp + fp + fn
        terms.append(2.0 * tp / den if den > 0 else 0.0)
    return float(np.mean(terms))


def micro_auroc(y_true, scores) -> float:
    """sklearn's roc_auc_score(one_hot(y_true), scores, average='micro'): ONE binary ROC AUC over the rows * C flattened
    (indicator, score) pairs -- the probability that a positive pair outscores a negative one, ties counting half:
    (sum of the positives' mid-ranks - n_pos (n_pos + 1) / 2) / (n_pos n_neg)."""
    scores = np.asarray(scores, dtype=np.float64)
    scores = scores.reshape(len(scores), -1)
    t = np.asarray(y_true).reshape(-1).astype(np.int64)
    hot = (t[:, None] == np.arange(scores.shape[1])[None, :]).reshape(-1)
    s = scores.reshape(-1)
    n_pos, n_neg = int(hot.sum()), int((~hot).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(s, kind="mergesort")
    ss = s[order]
    rank = np.empty(len(s), dtype=np.float64)
    start = np.flatnonzero(np.r_[True, ss[1:] != ss[:-1]])          # first position of every run of equal scores
    stop = np.r_[start[1:], len(ss)]
    for a, b in zip(start, stop):
        rank[order[a:b]] = 0.5 * (a + 1 + b)                        # mid-rank of positions a + 1 .. b
    return float((rank[hot].sum() - 0.5 * n_pos * (n_pos + 1)) / (float(n_pos) * float(n_neg)))


def expected_calibration_error(n_bins, logits, labels_true) -> float:
    """tfp.stats.expected_calibration_error(n_bins, logits, labels_true): softmax the logits, confidence_i = the
    softmax value at argmax_i (first maximum), bin_i = clip(floor(confidence_i * n_bins), 0, n_bins - 1),
    ECE = sum over non-empty bins of (count_b / rows) * |accuracy_b - mean confidence_b|."""
    z = np.asarray(logits, dtype=np.float64)
    z = z.reshape(len(z), -1)
    t = np.asarray(labels_true).reshape(-1).astype(np.int64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    prob = e / e.sum(axis=1, keepdims=True)
    pred = z.argmax(axis=1)
    conf = prob[np.arange(len(z)), pred]
    bins = np.clip(np.floor(conf * n_bins), 0, n_bins - 1).astype(np.int64)
    correct = (pred == t).astype(np.float64)
    ece = 0.0
    for b in range(int(n_bins)):
        sel = bins == b
        cnt = int(sel.sum())
        if cnt:
            ece += cnt / len(z) * abs(correct[sel].mean() - conf[sel].mean())
    return float(ece)


def two_columns(mean, m2=None, n_draws=None):
    """A one-output classifier read as q = [1 - p, p]: the mean becomes [1 - mean, mean]; with S1 = sum_s p = S mean and
    S2 = sum_s p^2 the second moment sum_s q q^T is [[S - 2 S1 + S2, S1 - S2], [S1 - S2, S2]].  Wider outputs pass
    through.  float64."""
    mean = np.asarray(mean, dtype=np.float64)
    mean = mean.reshape(len(mean), -1)
    if m2 is not None:
        m2 = np.asarray(m2, dtype=np.float64).reshape(len(mean), mean.shape[1], mean.shape[1])
    if mean.shape[1] != 1:
        return mean, m2
    out = np.concatenate([1.0 - mean, mean], axis=1)
    if m2 is None:
        return out, None
    s1, s2, S = float(n_draws) * mean[:, 0], m2[:, 0, 0], float(n_draws)
    q = np.empty((len(mean), 2, 2), dtype=np.float64)
    q[:, 0, 0] = S - 2.0 * s1 + s2
    q[:, 0, 1] = q[:, 1, 0] = s1 - s2
    q[:, 1, 1] = s2
    return out, q


def uncertainty_from_moments(mean, m2, n_draws, n_samples):
    """(total, aleatoric, epistemic), each (rows, C, C) float64, of Metrics.classification_uncertainty from the
    moments of the S = n_draws draws: mean (rows, C) = (1 / S) sum_s p_s, m2 (rows, C, C) = sum_s p_s p_s^T.

    The reference (Metrics.py:344-375) runs, for every draw s, over the rows j in order and ADDS to two running C x C
    matrices that it never resets inside a draw, appending the running value after every row; the per-draw lists are
    summed over the draws and divided by the ``n_samples`` ARGUMENT (the row count asked for, not the draw count).
    So entry j of each result is the sum over rows i <= j and over all draws of the per-(draw, row) term, / n_samples.

      aleatoric term:  diag(p) - p p^T.  Summed over the draws of row j, with S1 = sum_s p_s = S * mean_j, S2 = m2_j:
                       A_j = diag(S1) - S2.
      epistemic term:  d d^T with d = p.reshape(C, 1) - one_hot(label) -- a (C, 1) column minus a (C,) row, which
                       BROADCASTS to the C x C matrix d[a][b] = p_a - y_b.  (d d^T)[a][c] = sum_b (p_a - y_b)(p_c - y_b)
                       = C p_a p_c - (p_a + p_c) sum_b y_b + sum_b y_b^2 = C p_a p_c - p_a - p_c + 1, because a one-hot
                       row sums to 1 and so do its squares: the label drops out.  Summed over the draws:
                       E_j = C * S2 - S1 1^T - 1 S1^T + S 1 1^T.

    Returned: aleatoric = cumsum_j(A_j) / n_samples, epistemic = cumsum_j(E_j) / n_samples, total = their sum."""
    mean, m2 = two_columns(mean, m2, n_draws)
    S, C = float(n_draws), mean.shape[1]
    s1 = S * mean
    A = -m2.copy()
    idx = np.arange(C)
    A[:, idx, idx] += s1
    E = C * m2 - s1[:, :, None] - s1[:, None, :] + S
    aleatoric = np.cumsum(A, axis=0) / float(n_samples)
    epistemic = np.cumsum(E, axis=0) / float(n_samples)
    return epistemic + aleatoric, aleatoric, epistemic


# ---------------------------------------------------------------------------------------------------- the class
class Metrics:
    """Metrics(model, dataset): ``model`` a BayesianModel (or an optimizer's result() tuple, whose first entry is
    taken), ``dataset`` the Dataset whose split the metrics are computed on.

    Every method takes n_boundaries (weight draws of the Monte-Carlo mean), n_samples (the first n_samples rows of the
    split), data_type ("test", "train", anything else: validation) and save_path (writes <save_path>/report/<NAME>)."""

    def __init__(self, model, dataset):
        self._model = model[0] if isinstance(model, tuple) else model
        self._dataset = dataset
        self._cache = {}

    # ------------------------------------------------------------------ data and predictions
    def _get_x_y(self, n_samples=100, data_type="test"):
        split = self._dataset.valid_data
        if data_type == "test":
            split = self._dataset.test_data
        elif data_type == "train":
            split = self._dataset.train_data
        x, y_true = next(iter(split.batch(n_samples)))               # Metrics.py:341: the first batch of n_samples rows
        return np.asarray(x), np.asarray(y_true)

    def _get_predictions(self, x, n_boundaries, data_type):
        """The cached read-out of (n_boundaries, data_type, rows): {"mean": (rows, C) float64 (two columns for a
        one-output classifier), "m2": (rows, C, C) float64 or None (regression), "draws"}.  A miss costs one device
        read-out: predictive_moments (classification) or the mean-only predictive_mean (regression)."""
        key = (int(n_boundaries), data_type, len(x))
        hit = self._cache.get(key)
        if hit is None:
            if self._dataset.likelihood_model == "Classification":
                mean, m2, draws = self._model.predictive_moments(x, n_boundaries)
                mean, m2 = two_columns(mean, m2, draws)
            else:
                mean, m2 = np.asarray(self._model.predictive_mean(x, n_boundaries), dtype=np.float64), None
                draws = int(n_boundaries)
            hit = self._cache[key] = {"mean": mean, "m2": m2, "draws": draws}
        return hit

    def _read(self, n_boundaries, n_samples, data_type):
        x, y_true = self._get_x_y(n_samples=n_samples, data_type=data_type)
        return self._get_predictions(x, n_boundaries, data_type), y_true

    def _save(self, save_path, name, content):
        if save_path is not None:
            directory = os.path.join(save_path, "report")
            os.makedirs(directory, exist_ok=True)
            with open(os.path.join(directory, name), "w") as f:
                f.write(str(content))

    def _regression(self, what, fn, name, line, n_boundaries, n_samples, data_type, save_path):
        if self._dataset.likelihood_model == "Classification":
            raise Exception(what + " could only be computed for regression")
        pred, y_true = self._read(n_boundaries, n_samples, data_type)
        res = fn(y_true, pred["mean"])
        self._save(save_path, name, res)
        print(line.format(res))
        return res

    def _classification(self, fn, name, line, n_boundaries, n_samples, data_type, save_path):
        if self._dataset.likelihood_model != "Classification":
            raise Exception("Log likelihood could only be computed for regression")      # (the reference's message, as is)
        pred, y_true = self._read(n_boundaries, n_samples, data_type)
        res = fn(y_true, pred["mean"])
        self._save(save_path, name, res)
        print(line.format(res))
        return res

    # ------------------------------------------------------------------ summary
    def summary(self, n_boundaries: int = 30, n_samples: int = 100, data_type="test", save_path=None):
        """The reference's list for the likelihood model -- regression: mse, rmse, mae, r2, log_likeliood;
        classification: accuracy, recall, precision, f1_score, auroc, ece -- each printed (and saved); returns
        {method name: value}."""
        kw = dict(n_boundaries=n_boundaries, n_samples=n_samples, data_type=data_type, save_path=save_path)
        if self._dataset.likelihood_model == "Regression":
            names = ("mse", "rmse", "mae", "r2", "log_likeliood")
        elif self._dataset.likelihood_model == "Classification":
            names = ("accuracy", "recall", "precision", "f1_score", "auroc", "ece")
        else:
            print("Invalid loss function")
            return {}
        return {name: getattr(self, name)(**kw) for name in names}

    # ------------------------------------------------------------------ regression
    def mse(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """Mean squared error of the Monte-Carlo mean: mean over the output columns of mean_i (y_hat - y)^2."""
        return self._regression("Mean squared error", mean_squared_error, "MSE", "MSE: {}", n_boundaries, n_samples,
                                data_type, save_path)

    def rmse(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """Root mean squared error: sqrt(mean_i (y_hat - y)^2) per output column, then the columns' average."""
        return self._regression("Root mean squared error", root_mean_squared_error, "RMSE", "RMSE: {}", n_boundaries,
                                n_samples, data_type, save_path)

    def mae(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """Mean absolute error: mean over the output columns of mean_i |y_hat - y|."""
        return self._regression("Mean absolute error", mean_absolute_error, "MAE", "MAE: {}", n_boundaries, n_samples,
                                data_type, save_path)

    def r2(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """R2 = 1 - sum_i (y - y_hat)^2 / sum_i (y - mean y)^2 per output column, averaged; 1.0 / 0.0 for a column
        whose target is constant (predicted exactly / not)."""
        return self._regression("R2 score", r2_score, "R2", "R2 score: {}", n_boundaries, n_samples, data_type, save_path)

    def log_likeliood(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """(sic) mean of log N(y_hat; y, 1) = -(y_hat - y)^2 / 2 - log(2 pi) / 2 over rows and columns."""
        return self._regression("Log likelihood", gaussian_log_likelihood, "log_likelihood", "log likelihood: {}",
                                n_boundaries, n_samples, data_type, save_path)

    # ------------------------------------------------------------------ classification
    def accuracy(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """100 * share of rows whose argmax of the mean probabilities is the label."""
        return self._classification(lambda y, p: accuracy_score(y, p.argmax(axis=1)) * 100, "Accuracy", "Accuracy: {}%",
                                    n_boundaries, n_samples, data_type, save_path)

    def precision(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """As the reference computes it: 100 * macro RECALL (mean over the union of true and predicted labels of
        tp / (tp + fn), 0 for a label absent from the truth), under the name Precision."""
        return self._classification(lambda y, p: macro_recall(y, p.argmax(axis=1)) * 100, "Precision", "Precision: {}%",
                                    n_boundaries, n_samples, data_type, save_path)

    def recall(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """As the reference computes it: 100 * micro PRECISION (sum tp / sum (tp + fp) = the accuracy), under the
        name Recall."""
        return self._classification(lambda y, p: micro_precision(y, p.argmax(axis=1)) * 100, "Recall", "Recall: {}%",
                                    n_boundaries, n_samples, data_type, save_path)

    def f1_score(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None):
        """Macro F1: mean over the union of true and predicted labels of 2 tp / (2 tp + fp + fn); not x 100."""
        return self._classification(lambda y, p: macro_f1(y, p.argmax(axis=1)), "F1_score", "F1 score: {}", n_boundaries,
                                    n_samples, data_type, save_path)

    def ece(self, n_boundaries: int = 30, n_samples=100, data_type="test", save_path=None, n_bins=5):
        """Expected calibration error as the reference calls tfp's: the mean PROBABILITIES go in as logits, so they are
        softmaxed again; confidence = that value at the argmax, bin = clip(floor(confidence * n_bins), 0, n_bins - 1),
        ECE = sum_bins (count / rows) * |accuracy_bin - mean confidence_bin|."""
        return self._classification(lambda y, p: expected_calibration_error(n_bins, p, y), "ECE", "ECE: {}", n_boundaries,
                                    n_samples, data_type, save_path)

    def auroc(self, n_boundaries=10, n_samples=100, data_type="test", save_path=None, multi_class="ovr"):
        """Micro-averaged ROC AUC: one binary AUC over the rows * C flattened (one-hot label, mean probability) pairs,
        ties counting half.  ``multi_class`` is accepted as the reference passes it; the micro average of an indicator
        target does not depend on it."""
        if self._dataset.likelihood_model != "Classification":
            raise ValueError("ROC can only be plotted for Classification")
        pred, y_true = self._read(n_boundaries, n_samples, data_type)
        res = micro_auroc(y_true, pred["mean"])
        self._save(save_path, "AUROC", res)
        print("AUROC: {}".format(res))
        return res

    def classification_uncertainty(self, n_boundaries=30, n_samples=100, data_type="test", save_path=None):
        """(total, aleatoric, epistemic), each (rows, C, C) float64: ``uncertainty_from_moments`` (the derivation is
        there) of the device's per-row mean and second moment -- the reference's loop over every draw and every row
        without the loop and without the sample tensor."""
        if self._dataset.likelihood_model != "Classification":
            raise Exception("only for classification")
        pred, _ = self._read(n_boundaries, n_samples, data_type)
        return uncertainty_from_moments(pred["mean"], pred["m2"], pred["draws"], n_samples)
