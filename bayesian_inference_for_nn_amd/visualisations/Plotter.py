"""Plots of a trained ``BayesianModel`` over a ``Dataset`` (mirrors Pyesian/visualisations/Plotter.py): the same public
methods, keywords, defaults, exception types and messages, file names under ``<save_path>/report/plots``.

Every plotting method is split in two: a ``*_data`` method that returns the arrays, and a thin drawing part.  The
drawing part imports matplotlib when it is called (Agg when a figure is saved); without matplotlib it prints
"[Plotter] matplotlib unavailable; skipped <name>" and the data method still works.  sklearn, scikitplot and TensorFlow,
which the reference calls, are not imported; the functions below restate what those calls compute.

Where the numbers come from:
  * ``plot_decision_boundaries`` / ``plot_uncertainty_area`` read the posterior out on a dense 2-D grid (10^6 rows at
    granularity 1e-3).  The grid is made on the device and read out there (``BayesianModel.grid_surface``: pyz_grid_rows,
    pyz_predict_surface); one column per draw (the contour lines) or three numbers per row come back, never a grid row or
    the (draws, rows, C) sample tensor;
  * ``entropy``, ``confusion_matrix``, ``roc_one_vs_rest`` and the classification branch of
    ``compare_prediction_to_target`` use ``BayesianModel.predictive_surface`` (mean, argmax and entropy per row);
  * ``regression_uncertainty`` and the regression branch of ``compare_prediction_to_target`` use ``predict``'s samples
    and a float64 ``np.var`` on the host: a variance from float32 moments cancels when the spread is small against the
    mean, and the tensor is small here.

The reference is followed as it is written, quirks included (each named where it occurs):
  * ``plot_decision_boundaries`` hands n_boundaries=10 to its 2-D helper whatever the caller passed (:191-192);
  * ``plot_uncertainty_area`` uses ``n_samples`` as the number of weight draws too (:63) and does nothing for
    dimension != 2;
  * the scatter of ``plot_decision_boundaries`` shows classes 0 and 1 only (:111-112);
  * ``regression_uncertainty`` subtracts y_true from y_pred with the shapes they have (:246): targets of shape (rows,)
    broadcast against (rows, 1) predictions to rows x rows pairs.

Deviations, on purpose:
  * inputs wider than ``dimension``: the reference calls a ``tf.pca`` that does not exist (:94).  Here ``base_matrix``
    (d, 2) holds the first two PCA axes (``pca_axes``), the split is projected with ``x @ base_matrix`` and the grid is
    mapped back with ``grid @ base_matrix^T``, as :95 and :134 intend;
  * a one-output classifier is read as the two columns [1 - p, p] (``Metrics.two_columns``; the reference stacks them
    into a (rows, 2, 1) tensor on which argmax and sklearn fail);
  * ``roc_data`` keeps every distinct threshold (sklearn's ``roc_curve`` drops collinear points by default; the polyline
    drawn is the same); ``roc_one_vs_rest`` takes an optional ``save_path`` (the reference always shows the figure);
  * ``confusion_matrix`` draws what scikitplot's ``plot_confusion_matrix(normalize=True)`` draws, without its styling.
"""

from __future__ import annotations

import os

import numpy as np

from .Metrics import two_columns


# ---------------------------------------------------------------------------------------------------- host restatements
def pca_axes(x, k):
    """(d, k) float64: the first k principal axes of the rows of x as columns -- SVD of the centred matrix in float64, the
    sign of each axis fixed so that its largest-magnitude loading is positive."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(len(x), -1)
    if k > min(x.shape):
        raise ValueError(f"n_components={k} must be between 0 and min(n_samples, n_features)={min(x.shape)}")
    _, _, vt = np.linalg.svd(x - x.mean(axis=0), full_matrices=False)
    axes = vt[:k].copy()
    for c in axes:
        if c[np.argmax(np.abs(c))] < 0:
            c *= -1.0
    return axes.T


def pca_transform(x, k):
    """sklearn's PCA(n_components=k).fit_transform(x) up to the sign of each column: the centred rows on ``pca_axes``."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(len(x), -1)
    return (x - x.mean(axis=0)) @ pca_axes(x, k)


def grid_axes(x, granularity, un_zoom_level):
    """(a0, da, n1, b0, db, n2) of the grid of _extract_grid_x (:121-131) over the first two columns of x, in float32 as
    TensorFlow computes it: per axis size = max - min, start = min - (z / 2) size, limit = max + (z / 2) size,
    delta = granularity * (max - min + z * size), and tf.range's count ceil((limit - start) / delta)."""
    x = np.asarray(x, dtype=np.float32)
    f = np.float32
    out = []
    for k in (0, 1):
        hi, lo = x[:, k].max(), x[:, k].min()
        size = f(hi - lo)
        start = f(lo - f(f(un_zoom_level / 2) * size))
        limit = f(hi + f(f(un_zoom_level / 2) * size))
        delta = f(f(granularity) * f(f(hi - lo) + f(f(un_zoom_level) * size)))
        if not delta > 0:
            raise ValueError("the grid needs a positive step: a feature of the split is constant, or granularity <= 0")
        out += [float(start), float(delta), int(np.ceil(f(f(limit - start) / delta)))]
    return tuple(out)


def grid_mesh(a0, da, n1, b0, db, n2):
    """(dim1, dim2), each (n1, n2) float32: tf.meshgrid(indexing='ij') of u_i = a0 + i da and v_j = b0 + j db."""
    f = np.float32
    u = f(a0) + np.arange(n1, dtype=f) * f(da)
    v = f(b0) + np.arange(n2, dtype=f) * f(db)
    return np.meshgrid(u, v, indexing="ij")


def roc_curve(y_true, y_score):
    """(fpr, tpr, thresholds) of sklearn.metrics.roc_curve(y_true, y_score, drop_intermediate=False): the scores in
    descending order (stable), one point after the last row of every distinct score, (0, 0) with threshold inf in front.
    y_true is a 0 / 1 indicator.  NaN rates where a class is absent."""
    y = np.asarray(y_true).reshape(-1).astype(np.float64)
    s = np.asarray(y_score, dtype=np.float64).reshape(-1)
    order = np.argsort(-s, kind="mergesort")
    y, s = y[order], s[order]
    idx = np.r_[np.flatnonzero(np.diff(s)), len(s) - 1]
    tps = np.r_[0.0, np.cumsum(y)[idx]]
    fps = np.r_[0.0, 1.0 + idx - tps[1:]]
    with np.errstate(invalid="ignore", divide="ignore"):
        return fps / fps[-1], tps / tps[-1], np.r_[np.inf, s[idx]]


def confusion_counts(y_true, y_pred):
    """(labels, counts, normalised): labels = the sorted union of true and predicted labels, counts[i][j] = rows of true
    label i predicted as j, normalised = counts / row sums rounded to two decimals with NaN -> 0 (an empty row): what
    scikitplot's plot_confusion_matrix(normalize=True) draws."""
    t = np.asarray(y_true).reshape(-1).astype(np.int64)
    p = np.asarray(y_pred).reshape(-1).astype(np.int64)
    labels = np.union1d(t, p)
    counts = np.zeros((len(labels), len(labels)), dtype=np.int64)
    np.add.at(counts, (np.searchsorted(labels, t), np.searchsorted(labels, p)), 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = np.around(counts.astype(np.float64) / counts.sum(axis=1, keepdims=True), decimals=2)
    norm[np.isnan(norm)] = 0.0
    return labels, counts, norm


# ---------------------------------------------------------------------------------------------------- the class
class Plotter:
    """Plotter(model, dataset): ``model`` a BayesianModel (or an optimizer's result() tuple, whose first entry is taken),
    ``dataset`` the Dataset whose splits are plotted."""

    def __init__(self, model, dataset):
        self._model = model[0] if isinstance(model, tuple) else model
        self._dataset = dataset
        self._cache_key = None
        self._cached = None

    # ------------------------------------------------------------------ data and predictions
    def _get_x_y(self, n_samples=100, data_type="test"):
        """The first n_samples rows of the split (:80-87): "test", "train", anything else: validation."""
        split = self._dataset.valid_data
        if data_type == "test":
            split = self._dataset.test_data
        elif data_type == "train":
            split = self._dataset.train_data
        x, y_true = next(iter(split.batch(n_samples)))
        return np.asarray(x), np.asarray(y_true)

    def _get_predictions(self, x, n_boundaries, y_true, data_type):
        """The cached read-out (:32-52), keyed as the reference keys it: n_boundaries, the shape of y_true, data_type; one
        entry is kept.  Classification: {"mean" (rows, C) float64, two columns for a one-output model, "cls", "ent"} from
        predictive_surface; regression: {"samples" (draws, rows, C), "mean"} from predict."""
        key = (int(n_boundaries), tuple(np.shape(y_true)), data_type)
        if key != self._cache_key:
            if self._dataset.likelihood_model == "Classification":
                _, mean, _, cls, ent = self._model.predictive_surface(x, n_boundaries)
                hit = {"mean": two_columns(mean)[0], "cls": np.asarray(cls), "ent": np.asarray(ent)}
            else:
                samples, mean = self._model.predict(x, n_boundaries)
                hit = {"samples": np.asarray(samples), "mean": np.asarray(mean)}
            hit["x"], hit["y_true"] = x, y_true
            self._cache_key, self._cached = key, hit
        return self._cached

    def _read(self, n_boundaries, n_samples, data_type):
        x, y_true = self._get_x_y(n_samples, data_type)
        return self._get_predictions(x, n_boundaries, y_true, data_type)

    def _extract_x_y_from_dataset(self, dimension=2, n_samples=100, data_type="test"):
        """(x (rows, dimension), y, base_matrix (d, dimension)) (:89-98): the split as it is with the identity, or, for
        wider inputs, projected on its first PCA axes (the module docstring's first deviation)."""
        x, y = self._get_x_y(n_samples, data_type)
        x = np.asarray(x, dtype=np.float32).reshape(len(x), -1)
        if x.shape[1] > dimension:
            print("Dimension ", x.shape[1], " is not right.")
            print("Will apply PCA to reduce to dimension ", dimension)
            base_matrix = pca_axes(x, dimension).astype(np.float32)
            return x @ base_matrix, y, base_matrix
        elif x.shape[1] < dimension:
            raise ValueError("Dimension ", x.shape[1], " is inferior to given dimension")
        return x, y, np.eye(dimension, dtype=np.float32)

    def _extract_grid_x(self, x, granularity, un_zoom_level):
        a0, da, n1, b0, db, n2 = grid = grid_axes(x, granularity, un_zoom_level)
        dim1, dim2 = grid_mesh(a0, da, n1, b0, db, n2)
        return grid, dim1, dim2

    # ------------------------------------------------------------------ decision surfaces
    def decision_boundaries_data(self, dimension=2, granularity=1e-2, n_boundaries=30, n_samples=100, data_type="test",
                                 un_zoom_level=0.2):
        """{"x", "y", "base_matrix", "dim1", "dim2" (n1, n2), "boundaries" (10, n1, n2), "n_boundaries": 10}: column 0 of
        ten weight draws' predictions on the grid -- ten, whatever n_boundaries says (:191-192)."""
        if self._dataset.likelihood_model != "Classification":
            raise ValueError("Decision boundary can only be plotted for Classification")
        x, y, base_matrix = self._extract_x_y_from_dataset(dimension=dimension, n_samples=n_samples, data_type=data_type)
        if dimension != 2:
            raise ValueError("Decision boundary can only be plotted in 2 dimensions")
        n_boundaries = 10
        grid, dim1, dim2 = self._extract_grid_x(x, granularity, un_zoom_level)
        cols = self._model.grid_surface(base_matrix, *grid, n_boundaries, column=0, want_cols=True)[0]
        return {"x": x, "y": np.asarray(y).reshape(-1), "base_matrix": base_matrix, "dim1": dim1, "dim2": dim2,
                "boundaries": cols.reshape((n_boundaries,) + dim1.shape), "n_boundaries": n_boundaries}

    def plot_decision_boundaries(self, dimension=2, granularity=1e-2, n_boundaries=30, n_samples=100, data_type="test",
                                 un_zoom_level=0.2, save_path=None):
        """Ten decision boundaries (the 0.5 contour of column 0 of ten weight draws) over the scatter of classes 0 and 1.
        ValueError for other than classification and for dimension != 2."""
        d = self.decision_boundaries_data(dimension, granularity, n_boundaries, n_samples, data_type, un_zoom_level)
        plt = self._pyplot("decision_boundaries", save_path)
        if plt is None:
            return
        x, y = d["x"], d["y"]
        plt.figure(figsize=(8, 6))
        plt.scatter(x[y == 0][:, 0], x[y == 0][:, 1], marker="o", c="blue", label="Class 0")
        plt.scatter(x[y == 1][:, 0], x[y == 1][:, 1], marker="x", c="red", label="Class 1")
        for pred in d["boundaries"]:
            if pred.min() < 0.5 < pred.max():           # (a draw whose boundary misses the window has no contour)
                plt.contour(d["dim1"], d["dim2"], pred, [0.5], colors=["red"])
        plt.legend()
        plt.xlabel("Feature 1")
        plt.ylabel("Feature 2")
        plt.title("Multiple Decision Boundaries N=" + str(d["n_boundaries"]))
        self._save(plt, save_path, "decision_boundaries") if save_path else plt.show()

    def uncertainty_area_data(self, dimension=2, granularity: float = 1e-2, n_samples=100, data_type="test",
                              uncertainty_threshold=0.8, un_zoom_level=0.2):
        """{"x", "y", "classes", "base_matrix", "dim1", "dim2", "top", "uncertain" (n1, n2)}: top = the largest mean
        probability of n_samples weight draws (:63: the row count doubles as the draw count) at every grid point,
        uncertain = 1.0 where top < uncertainty_threshold (in float32).  None for dimension != 2."""
        if self._dataset.likelihood_model != "Classification":
            raise ValueError("Uncertainty area can only be plotted for Classification")
        x, y, base_matrix = self._extract_x_y_from_dataset(dimension=dimension, n_samples=n_samples, data_type=data_type)
        if dimension != 2:
            return None
        grid, dim1, dim2 = self._extract_grid_x(x, granularity, un_zoom_level)
        top = self._model.grid_surface(base_matrix, *grid, n_samples, column=0, want_cols=False)[2].reshape(dim1.shape)
        y = np.asarray(y).reshape(-1)
        return {"x": x, "y": y, "classes": np.unique(y), "base_matrix": base_matrix, "dim1": dim1, "dim2": dim2, "top": top,
                "uncertain": (top < np.float32(uncertainty_threshold)).astype(np.float32)}

    def plot_uncertainty_area(self, dimension=2, granularity: float = 1e-2, n_samples=100, data_type="test",
                              uncertainty_threshold=0.8, un_zoom_level=0.2, save_path=None):
        """The area where the largest mean probability is below uncertainty_threshold, over the scatter of every class.
        ValueError for other than classification; nothing for dimension != 2."""
        d = self.uncertainty_area_data(dimension, granularity, n_samples, data_type, uncertainty_threshold, un_zoom_level)
        if d is None:
            return
        plt = self._pyplot("uncertainty_area", save_path)
        if plt is None:
            return
        x, y = d["x"], d["y"]
        plt.figure()
        for i in range(len(d["classes"])):              # :64-67: labels 0 .. n_classes - 1
            plt.scatter(x[y == i][:, 0], x[y == i][:, 1], marker="o", label="Class " + str(i))
        if d["uncertain"].max() > 0.9:                  # (no uncertain point: no area to fill)
            plt.contourf(d["dim1"], d["dim2"], d["uncertain"], [0.9, 1.1], colors=["orange"], alpha=0.5)
        plt.xlabel("Feature 1")
        plt.ylabel("Feature 2")
        plt.legend()
        plt.title("Uncertainty area with threshold " + str(uncertainty_threshold))
        self._save(plt, save_path, "uncertainty_area") if save_path else plt.show()

    # ------------------------------------------------------------------ ROC
    def roc_data(self, n_samples=100, label_of_interest: int = 0, n_boundaries=10, data_type="test"):
        """(fpr, tpr, thresholds) of label_of_interest against the rest on the mean probabilities: ``roc_curve`` above,
        every distinct threshold kept."""
        if self._dataset.likelihood_model != "Classification":
            raise ValueError("ROC can only be plotted for Classification")
        pred = self._read(n_boundaries, n_samples, data_type)
        y_true = np.asarray(pred["y_true"]).reshape(-1)
        return roc_curve(y_true == label_of_interest, pred["mean"][:, label_of_interest])

    def roc_one_vs_rest(self, n_samples=100, label_of_interest: int = 0, n_boundaries=10, data_type="test", save_path=None):
        """The ROC curve of one label against the rest, with the chance level.  ValueError for other than classification."""
        fpr, tpr, _ = self.roc_data(n_samples, label_of_interest, n_boundaries, data_type)
        plt = self._pyplot("roc_one_vs_rest", save_path)
        if plt is None:
            return
        auc = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))
        plt.figure()
        plt.plot(fpr, tpr, color="blue", label=f"class {label_of_interest} vs the rest (AUC = {auc:.2f})")
        plt.plot([0, 1], [0, 1], "k--", label="Chance level (AUC = 0.5)")
        plt.xlabel("False Positive Rate")
        plt.ylabel("True Positive Rate")
        plt.title("ROC curve One-vs-Rest")
        plt.legend()
        self._save(plt, save_path, "roc_one_vs_rest") if save_path else plt.show()

    # ------------------------------------------------------------------ regression
    def regression_uncertainty_data(self, n_boundaries=30, n_samples=100, data_type="test"):
        """(pred_dev, err) of :244-246: err = the mean over the output columns of the standard deviation of the draws
        (np.var in float64), pred_dev = np.mean(y_pred - y_true, axis=1) with the shapes the two have."""
        if self._dataset.likelihood_model != "Regression":
            raise ValueError("regression uncertainty cannot be computed for other than regression problems")
        pred = self._read(n_boundaries, n_samples, data_type)
        variance = np.var(np.asarray(pred["samples"], dtype=np.float64), axis=0)
        err = np.mean(np.sqrt(variance), axis=1)
        pred_dev = np.mean(np.asarray(pred["mean"]) - np.asarray(pred["y_true"]), axis=1)
        return pred_dev, err

    def regression_uncertainty(self, n_boundaries=30, n_samples=100, data_type="test", save_path=None):
        """The deviation of the mean prediction from the target with the epistemic band around it.  ValueError for other
        than regression."""
        pred_dev, err = self.regression_uncertainty_data(n_boundaries, n_samples, data_type)
        plt = self._pyplot("epistemic_uncertainty", save_path)
        if plt is None:
            return
        plt.figure(figsize=(10, 5))
        plt.hlines([0], 0, len(err))
        plt.plot(range(len(err)), pred_dev - err, label="Epistemic Lower", alpha=0.5)
        plt.scatter(range(len(err)), pred_dev, label="Averaged deviation", alpha=0.5, c="k")
        plt.plot(range(len(err)), pred_dev + err, label="Epistemic Upper", alpha=0.5)
        plt.legend()
        plt.title("Epistemic Uncertainty")
        plt.ylabel("Pred-True difference")
        self._save(plt, save_path, "epistemic_uncertainty") if save_path else plt.show()

    # ------------------------------------------------------------------ classification
    def confusion_matrix_data(self, n_boundaries=30, n_samples=100, data_type="test"):
        """(labels, counts, normalised) of ``confusion_counts`` for the argmax of the mean probabilities."""
        if self._dataset.likelihood_model != "Classification":
            raise ValueError("Confusion matrix cannot be computed for other than classification problems")
        pred = self._read(n_boundaries, n_samples, data_type)
        return confusion_counts(pred["y_true"], pred["cls"])

    def confusion_matrix(self, n_boundaries=30, n_samples=100, data_type="test", save_path=None):
        """The row-normalised confusion matrix.  ValueError for other than classification."""
        labels, _, norm = self.confusion_matrix_data(n_boundaries, n_samples, data_type)
        plt = self._pyplot("confusion_matrix", save_path)
        if plt is None:
            return
        fig, ax = plt.subplots()
        image = ax.imshow(norm, interpolation="nearest", cmap="Blues")
        fig.colorbar(image)
        ax.set_xticks(range(len(labels)))
        ax.set_yticks(range(len(labels)))
        ax.set_xticklabels(labels)
        ax.set_yticklabels(labels)
        for i in range(len(labels)):
            for j in range(len(labels)):
                ax.text(j, i, norm[i, j], ha="center", va="center", color="white" if norm[i, j] > norm.max() / 2 else "black")
        ax.set_xlabel("Predicted label")
        ax.set_ylabel("True label")
        ax.set_title("Confusion Matrix")
        self._save(plt, save_path, "confusion_matrix") if save_path else plt.show()

    def entropy_data(self, n_boundaries=30, n_samples=100, data_type="test"):
        """The entropies -sum_a q_a log(q_a + 1e-5) of the mean rows (float32, computed on the device), nan_to_num'd, then
        sorted (:364-367).  A plain Exception for other than classification, as the reference raises."""
        if self._dataset.likelihood_model != "Classification":
            raise Exception("Entropy is only available for classification")
        pred = self._read(n_boundaries, n_samples, data_type)
        return np.sort(np.nan_to_num(pred["ent"]))

    def entropy(self, n_boundaries=30, n_samples=100, data_type="test", save_path=None):
        """The sorted entropies of the mean predictions."""
        entropies = self.entropy_data(n_boundaries, n_samples, data_type)
        plt = self._pyplot("entropy", save_path)
        if plt is None:
            return
        plt.figure()
        plt.plot(range(len(entropies)), entropies)
        plt.title("Entropies for each input")
        plt.xlabel("Sample Index")
        plt.ylabel("entropy")
        self._save(plt, save_path, "entropy") if save_path else plt.show()

    def compare_prediction_to_target_data(self, n_boundaries=30, n_samples=100, data_type="test"):
        """Regression: {"kind": "regression", "y_true" (reshaped to y_pred's shape), "y_pred"}.  Classification:
        {"kind": "2d" or "3d", "x", "y_true", "y_pred"}: the predicted labels and the inputs -- as they are when they have
        two columns, else on their first three PCA axes (two for inputs narrower than three), centred, float64 (:310-320)."""
        pred = self._read(n_boundaries, n_samples, data_type)
        if self._dataset.likelihood_model == "Regression":
            y_pred = np.asarray(pred["mean"])
            return {"kind": "regression", "y_true": np.asarray(pred["y_true"]).reshape(y_pred.shape), "y_pred": y_pred}
        x_2d = np.asarray(pred["x"]).reshape(len(pred["x"]), -1)
        if x_2d.shape[1] == 2:
            kind, x = "2d", x_2d
        elif x_2d.shape[1] >= 3:
            kind, x = "3d", pca_transform(x_2d, 3)
        else:
            kind, x = "2d", pca_transform(x_2d, 2)
        return {"kind": kind, "x": x, "y_true": np.asarray(pred["y_true"]).reshape(-1), "y_pred": pred["cls"]}

    def compare_prediction_to_target(self, n_boundaries=30, n_samples=100, data_type="test", save_path=None):
        """True against predicted values (regression with one output column) or labels (classification, over the inputs or
        their PCA projection)."""
        d = self.compare_prediction_to_target_data(n_boundaries, n_samples, data_type)
        if d["kind"] == "regression" and d["y_true"].shape[1] != 1:
            return
        plt = self._pyplot("comparison_pred_true", save_path)
        if plt is None:
            return
        y_true, y_pred = d["y_true"], d["y_pred"]
        if d["kind"] == "regression":
            plt.figure(figsize=(10, 5))
            plt.scatter(range(len(y_true)), y_true, label="True Values", alpha=0.5)
            plt.scatter(range(len(y_pred)), y_pred, label="Predicted Mean", alpha=0.5)
            plt.legend()
            plt.title("True vs Predicted Values")
            plt.xlabel("Sample Index")
            plt.ylabel("Output")
        elif d["kind"] == "2d":
            x = d["x"]
            fig, (ax_true, ax_pred) = plt.subplots(2, figsize=(12, 8))
            for ax, c in ((ax_true, y_true), (ax_pred, y_pred)):
                scatter = ax.scatter(x[:, -2], x[:, -1], c=c, s=5)
                ax.add_artist(ax.legend(*scatter.legend_elements(), loc="lower left", title="Digits"))
            ax_true.set_title("First Two Dimensions of Projected True Data After Applying PCA")
            ax_pred.set_title("First Two Dimensions of Projected Predicted Data After Applying PCA")
        else:
            x = d["x"]
            fig = plt.figure(figsize=plt.figaspect(0.5))
            for k, c in ((1, y_true), (2, y_pred)):
                ax = fig.add_subplot(1, 2, k, projection="3d")
                fig.colorbar(ax.scatter(x[:, -3], x[:, -2], x[:, -1], c=c, s=1), shrink=0.5)
            plt.title("First Three Dimensions of Projected True Data (left) VS Predicted Data (right) After Applying PCA")
        self._save(plt, save_path, "comparison_pred_true") if save_path else plt.show()

    # ------------------------------------------------------------------ training
    def learning_diagnostics(self, loss_file: str, save_path=None):
        """The training losses of a text file (one per line), against the iteration."""
        if loss_file is None:
            return
        losses = np.loadtxt(loss_file)
        plt = self._pyplot("learning_diagnostics", save_path)
        if plt is None:
            return
        plt.figure()
        plt.plot(losses, label="Loss")
        plt.title("Training Loss")
        plt.xlabel("Iterations")
        plt.ylabel("Loss")
        plt.legend()
        self._save(plt, save_path, "learning_diagnostics") if save_path else plt.show()

    # ------------------------------------------------------------------ drawing
    @staticmethod
    def _pyplot(name, save_path):
        try:
            import matplotlib
            if save_path:
                matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except Exception:
            print(f"[Plotter] matplotlib unavailable; skipped {name}")
            return None
        return plt

    @staticmethod
    def _save(plt, save_path, name):
        plots = os.path.join(save_path, "report", "plots")                   # Plotter.py:395-400
        os.makedirs(plots, exist_ok=True)
        plt.savefig(os.path.join(plots, name + ".png"))
        plt.close()
