"""Robustness of a trained ``BayesianModel`` (mirrors Pyesian/visualisations/Robustness.py).

Adversarial (:115-144): an FGSM attack on the whole validation split along the loss gradient summed over weight draws, then
a Monte-Carlo prediction on the perturbed inputs.  The gradient, its sum over the draws and the FGSM step run on the device
(pyz_input_grad).

Corruption (:10-93, :147-273): ``mean_corruption_error``, ``corruption_error``, ``robustness_by_corruption`` and
``corruption_robustness_by_severity`` over the nine image corruptions (classification) or Gaussian input noise
(regression) at severities 1..5.  The reference corrupts image by image in Python through PIL and skimage; here, per
corruption, the clean split is uploaded once, the five corrupted copies of it are made by one kernel per corruption (pyz_corrupt_rows, the
reference functions restated without PIL or skimage: include/pyz.h), read out like ``predict`` and scored on the device
(pyz_score_rows): per corruption five numbers come back (``BayesianModel.corruption_scores``).  The noise is the
library's Philox stream under ``seed``, not NumPy's global one.  These measures are ``CorruptionMeasures``, an object of
its own with the cache and the seed; every ``Robustness`` instance makes one and carries its four methods and its
``corruptions`` / ``corruption_dict`` / ``error_dict`` / ``severities`` under the reference's names."""

from __future__ import annotations

import os

import numpy as np

from .. import losses
from .Metrics import two_columns

CORRUPTIONS = ("gaussian_noise", "shot_noise", "impulse_noise", "speckle_noise", "gaussian_blur", "contrast", "brightness",
               "saturate", "pixelate")       # Robustness.py:103-104, in the order of the kernel's kind ids 0..8
REGRESSION_NOISE = 9                         # gaussian_noise_regression (:16-19)


def _save_data(path, name, content):
    report = os.path.join(path, "report", "robustness")                  # Robustness.py:282-288
    os.makedirs(report, exist_ok=True)
    with open(os.path.join(report, name + ".txt"), "w") as f:
        f.write(str(content))


class CorruptionMeasures:
    """The corruption half of the reference class (Robustness.py:147-273) over one model and one split (x, y_true)."""

    METHODS = ("mean_corruption_error", "corruption_error", "robustness_by_corruption", "corruption_robustness_by_severity")
    ATTRIBUTES = ("corruptions", "corruption_dict", "error_dict", "n", "severities", "pixel_max", "seed")

    def __init__(self, model, regression, x, y_true, pixel_max=255.0, seed=None):
        self.model, self.regression, self.x, self.y_true = model, regression, x, y_true
        self.corruptions = CORRUPTIONS
        self.corruption_dict = {name: kind for kind, name in enumerate(self.corruptions)}
        self.error_dict = {name: None for name in self.corruptions}     # per-severity FRACTIONS wrong, once per corruption
        self.n = len(self.corruptions)
        self.severities = np.arange(1, 6)
        self.pixel_max = float(pixel_max)
        self.seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if seed is None else int(seed)

    def mean_corruption_error(self, relative=False, nb_samples=100, save_path=None):
        """The mean (relative) corruption error over all corruptions and severities (Robustness.py:147-168): printed, or
        written to <save_path>/report/robustness/mean_corruption_error.txt (mean_relative_error.txt); also returned.
        nb_samples reaches the read-outs (the reference drops it there and reads out with its default, the same 100)."""
        if self.regression:
            # :157-158: regression has one entry, the input noise
            ce = np.array([self.corruption_error(helper=True, relative=relative, nb_boundaries=nb_samples)])
        else:
            # :160: the average of corruption_error(..., helper=True) over the nine names
            ce = np.array([self.corruption_error(c, helper=True, relative=relative, nb_boundaries=nb_samples)
                           for c in self.corruption_dict.keys()])
        mean = float(np.mean(ce))
        if save_path:
            _save_data(save_path, "mean_relative_error" if relative else "mean_corruption_error", mean)
        else:
            name = "Mean Relative Error: " if relative else "Mean Corruption Error: "
            print(name + str(mean) if self.regression else name + str(mean) + " %")
        return mean

    def corruption_error(self, corruption=None, relative=False, nb_boundaries=100, save_path=None, helper=False):
        """The (relative) corruption error of one corruption over the five severities (Robustness.py:170-202), in percent
        for classification: returned (helper=True: silently), else also printed or written to
        <save_path>/report/robustness/corruption_error_<corruption>.txt (relative_error_<corruption>.txt)."""
        error = self._severity_errors(corruption, nb_boundaries)
        if not self.regression:
            error = error * 100                     # :187: classification errors are in percent
        if relative:
            # :190-192: the clean error is an RMSE or a FRACTION, subtracted as it is from the percentages
            ce = float(np.sum(error - self._clean_error(nb_boundaries)) / len(self.severities))
        else:
            ce = float(np.sum(error) / len(self.severities))   # :194: the sum over the five severities, divided by 5
        if helper:
            return ce
        name = corruption if corruption is not None else "noise"
        if save_path:
            _save_data(save_path, ("relative_error_" if relative else "corruption_error_") + name, ce)
        else:
            print_stat = "Relative Error for {}: {}%" if relative else "Corruption Error for {}: {}%"
            print(print_stat.format(name, ce))
        return ce

    def robustness_by_corruption(self, nb_samples=100, save_path=None):
        """The corruption error of every corruption as a bar graph (Robustness.py:204-214), saved to
        <save_path>/report/robustness/figures/robustness_by_corruption.png or shown; the nine values are returned."""
        ce = np.array([self.corruption_error(c, nb_boundaries=nb_samples, helper=True) for c in self.corruption_dict.keys()])
        plt = self._pyplot("robustness_by_corruption", save_path)
        if plt is not None:
            plt.figure()
            plt.bar(list(self.corruption_dict.keys()), ce)
            plt.xlabel("Corruption")
            plt.ylabel("Corruption Error" if self.regression else "Corruption Error (%)")
            plt.title("Corruption Error by Corruption")
            self._save_figure(plt, save_path, "robustness_by_corruption") if save_path else plt.show()
        return ce

    def corruption_robustness_by_severity(self, corruption=None, nb_samples=100, save_path=None):
        """The error of one corruption at each severity as a bar graph (Robustness.py:216-233), in percent for
        classification (the axis label's unit), saved to
        <save_path>/report/robustness/figures/corruption_robustness_by_severity.png or shown; the five values are returned."""
        error = self._severity_errors(corruption, nb_samples)
        if not self.regression:
            error = error * 100
        plt = self._pyplot("corruption_robustness_by_severity", save_path)
        if plt is not None:
            plt.figure()
            plt.bar(self.severities, error)
            plt.xlabel("Severity")
            plt.ylabel("Error Rate" if self.regression else "Error Rate (%)")
            plt.title("Error Rate by Severity for {}".format("noise" if self.regression else corruption))
            self._save_figure(plt, save_path, "corruption_robustness_by_severity") if save_path else plt.show()
        return error

    def _image_shape(self):
        shape = tuple(int(d) for d in np.shape(self.x)[1:])
        if len(shape) == 2:
            return shape + (1,)
        if len(shape) == 3 and shape[2] in (1, 3):
            return shape
        raise ValueError(f"the corruptions need images of shape (H, W), (H, W, 1) or (H, W, 3), not {shape}")

    def _severity_errors(self, corruption, nb_samples):
        """float64 (5,): the fraction of rows wrong (classification, cached per corruption) or the RMSE (regression) at
        severities 1..5 (Robustness.py:235-256)."""
        if self.regression:
            # :181,237-238: regression ignores `corruption`: Gaussian noise on every input column, not cached
            row = (1, int(np.prod(np.shape(self.x)[1:])), 1)
            return np.asarray(self.model.corruption_scores(self.x, self.y_true, row, REGRESSION_NOISE, self.severities,
                                                           nb_samples, True, self.pixel_max, self.seed), dtype=np.float64)
        if corruption not in self.corruption_dict:
            raise KeyError(f"unknown corruption {corruption!r}: one of {', '.join(self.corruptions)}")
        if self.error_dict[corruption] is None:
            self.error_dict[corruption] = np.asarray(
                self.model.corruption_scores(self.x, self.y_true, self._image_shape(), self.corruption_dict[corruption],
                                             self.severities, nb_samples, False, self.pixel_max, self.seed), dtype=np.float64)
        return self.error_dict[corruption]

    def _clean_error(self, nb_samples):
        """RMSE (regression) or 1 - accuracy as a fraction (classification) of a read-out of the clean split (:190-191)."""
        predicted = np.asarray(self.model.predictive_mean(self.x, nb_samples), dtype=np.float64)
        if self.regression:
            y = np.asarray(self.y_true, dtype=np.float64).reshape(len(predicted), -1)
            return float(np.sqrt(((predicted.reshape(y.shape) - y) ** 2).mean(axis=0)).mean())
        predicted = two_columns(predicted.reshape(len(predicted), -1))[0]
        return 1.0 - float((predicted.argmax(axis=1) == np.asarray(self.y_true).reshape(-1)).mean())

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
    def _save_figure(plt, path, name):
        figures = os.path.join(path, "report", "robustness", "figures")      # Robustness.py:275-280
        os.makedirs(figures, exist_ok=True)
        plt.savefig(os.path.join(figures, name + ".png"))
        plt.close()



class Robustness:
    def __init__(self, model, dataset, pixel_max=255.0, seed=None):
        self.model = model[0] if isinstance(model, tuple) else model    # (an optimizer's result() tuple works too)
        self.dataset = dataset
        self.regression = dataset.likelihood_model == "Regression"
        self.x, self.y_true = dataset.valid_data.as_numpy()             # Robustness.py:110: one batch = the whole split
        # the corruption measures are bound per instance: the class itself holds the adversarial measure alone
        self.corruption = CorruptionMeasures(self.model, self.regression, self.x, self.y_true, pixel_max, seed)
        for name in CorruptionMeasures.METHODS + CorruptionMeasures.ATTRIBUTES:
            setattr(self, name, getattr(self.corruption, name))

    def adversarial_robustness(self, epsilon=0.1, nb_samples=100, save_path=None):
        """Accuracy x 100 (classification) or RMSE (regression) of the mean prediction on x + epsilon * sign(sum over
        nb_samples draws of d loss / d x).  Printed, or written to <save_path>/report/robustness/adversarial_robustness.txt;
        also returned."""
        kind = losses.loss_kind(self.dataset._loss)
        # one set of draws for the gradient (Robustness.py:127-136); predict then draws its own (:139)
        x_adv, _ = self.model.adversarial_examples(self.x, self.y_true, kind, epsilon, nb_samples)
        _, predicted = self.model.predict(x_adv, nb_samples)
        predicted = np.asarray(predicted, dtype=np.float64)
        if self.regression:
            y = np.asarray(self.y_true, dtype=np.float64).reshape(len(predicted), -1)
            # sklearn's root_mean_squared_error: per output column, then their plain average
            robustness = float(np.sqrt(((predicted.reshape(y.shape) - y) ** 2).mean(axis=0)).mean())
            stat = "Adversarial Robustness: " + str(robustness)
        else:
            y = np.asarray(self.y_true).reshape(-1)
            # one output column is read as [1 - p, p], like Metrics: class 1 where the mean exceeds 0.5 (the reference's
            # argmax over the single column is class 0 for every row)
            predicted = two_columns(predicted.reshape(len(predicted), -1))[0]
            robustness = float((predicted.argmax(axis=1) == y).mean()) * 100
            stat = "Adversarial Robustness: " + str(robustness) + "%"
        _save_data(save_path, "adversarial_robustness", robustness) if save_path else print(stat)
        return robustness
