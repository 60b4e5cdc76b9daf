"""Adversarial robustness of a trained ``BayesianModel`` (mirrors Pyesian/visualisations/Robustness.py:115-144): an
FGSM attack on the whole validation split along the loss gradient summed over weight draws, then a Monte-Carlo
prediction on the perturbed inputs.  The gradient, its sum over the draws and the FGSM step run on the device
(pyz_input_grad).  The corruption-based measures of the reference class (host-side image processing) are not part of it."""

from __future__ import annotations

import os

import numpy as np

from .. import losses
from .Metrics import two_columns


class Robustness:
    def __init__(self, model, dataset):
        self.model = model[0] if isinstance(model, tuple) else model    # (an optimizer's result() tuple works too)
        self.dataset = dataset
        self.regression = dataset.likelihood_model == "Regression"
        self.x, self.y_true = dataset.valid_data.as_numpy()             # Robustness.py:110: one batch = the whole split

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
        if save_path:
            report = os.path.join(save_path, "report", "robustness")
            os.makedirs(report, exist_ok=True)
            with open(os.path.join(report, "adversarial_robustness.txt"), "w") as f:
                f.write(str(robustness))
        else:
            print(stat)
        return robustness
