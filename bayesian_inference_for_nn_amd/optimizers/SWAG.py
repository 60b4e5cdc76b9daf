"""SWAG (mirrors Pyesian/optimizers/SWAG.py:13-149): SGD steps from a starting model plus running
first / second moments and a k-column deviation matrix; posterior =
MultivariateNormalDiagPlusLowRank per layer.  Hyperparameters: batch_size, lr, k, scale, frequency;
kwarg starting_model.  One fused device step (the update, the moments and the deviation row are
written in the epilogue of the weight-gradient kernel).

Extension: kwarg n_members = P > 1 trains P SWAG models in one particle-batched step -- MultiSWAG (Wilson & Izmailov
2020); the reference trains one, and n_members absent or 1 is that path, untouched.  starting_model may be a list of P
models (member c copies entry c: SWAG(starting_model=sgd.member_models())) or one model (member 0 copies it, member
c >= 1 starts from the Glorot draw of seed + c).  All members of a rank see the rank's minibatches, like SGLD's chains:
the diversity comes from the starts.  member_results() gives one BayesianModel per member, built as result() builds
the one.  result() is one model with ONE distribution over all weight layers: a Mixture of P
MultivariateNormalDiagPlusLowRank components, each over all D weights, so that a draw takes every layer from the same
member.  A deviation from the per-layer result of one SWAG: a component draws one z2 for all layers, where the
one-member result draws a z2 per layer.  The net's weights are member 0's.  With several ranks result() is the rank's
own: members are not merged across ranks."""

from math import sqrt

import numpy as np

from ..distributions.MultivariateNormalDiagPlusLowRank import MultivariateNormalDiagPlusLowRank
from ..nn import BayesianModel
from . import _members
from .Optimizer import DeviceScalar, Optimizer


class SWAG(Optimizer):
    _conv_models = True      # a model with Conv2D layers trains through step(), one member

    def __init__(self):
        super().__init__()
        self._n = None
        self._lr = None
        self._frequency = None
        self._k = None
        self._n_members = 1

    def compile_extra_components(self, **kwargs):
        """A plan for P = n_members particles; the state is (D,) with (k, D) deviation rows for one member, the
        reference's path, and (P, D) with (P, k, D) rows for several (see the module docstring for the starts)."""
        import torch
        P = self._n_members = _members.n_members_of(kwargs)
        self._k = int(self._hyperparameters.k)
        self._frequency = int(self._hyperparameters.frequency)
        self._lr = self._hyperparameters.lr
        self._scale = self._hyperparameters.scale
        self._batch_size = int(self._hyperparameters.batch_size)
        start = kwargs["starting_model"]
        _members.check_starts(start, P)
        self._setup_backend(seed=kwargs.get("seed"), max_particles=P, chains_per_rank=P)
        rows = _members.member_starts(self, start, P)          # SWAG.py:107-108: the starting model's weights are copied
        self._theta = torch.as_tensor(rows if P > 1 else rows[0]).cuda()
        self._base_model = self._net
        self._dataset_setup()
        lead = (P,) if P > 1 else ()
        self._mean_dev = torch.zeros(lead + (self._D,), device="cuda")     # SWAG.py:113-127
        self._sq_mean_dev = torch.zeros(lead + (self._D,), device="cuda")
        # row r (of member c) = column r of the reference's (member c's) matrix
        self._dev_rows = torch.zeros(lead + (self._k, self._D), device="cuda")
        self._n_cols = 0
        self._loss_dev = torch.zeros(P, device="cuda")
        self._loss_cols = P if P > 1 else None                 # a loss per member and step
        self._weight_layers_indices = self._layer_indices()
        self._n = 0

    def step(self, save_document_path=None):
        idx, b, _ = self._next_batch()
        update = self._n % self._frequency == 0                             # SWAG.py:72
        # columns are appended until there are k; afterwards the LAST one is replaced (SWAG.py:85-89, as written)
        col = min(self._n_cols, self._k - 1)
        if self._n_members > 1:
            self._plan.swag_members_step(self._theta, self._mean_dev, self._sq_mean_dev, self._dev_rows, self._x_dev,
                                         self._y_dev, self._lr, self._n, update, col if update else None, self._loss_dev,
                                         batch=b, row_idx=idx)
            loss = self._loss_dev.mean().reshape(1)            # the mean over members of the batch loss
        else:
            self._plan.swag_step(self._theta, self._mean_dev, self._sq_mean_dev, self._dev_rows[col] if update else None,
                                 self._x_dev, self._y_dev, self._lr, self._n, update, self._loss_dev, batch=b, row_idx=idx)
            loss = self._loss_dev.clone()
        if update and self._n_cols < self._k:
            self._n_cols += 1
        if save_document_path != None:
            self._append_loss(save_document_path, str(float(loss.item())))
        self._n += 1
        return DeviceScalar(loss, 0)

    # ------------------------------------------------------------------ quiet train(): device-resident runs
    def _resident_supported(self):
        return not self._conv and (self._n_members > 1 or self._fused_head())

    def _resident_launch(self, nb_iterations):
        """The moment / deviation-column bookkeeping is a function of the step count and runs on the device (the chain
        starts at count 0: compile sets it)."""
        run = self._plan.swag_members_run if self._n_members > 1 else self._plan.swag_run

        def launch(idx, losses, sizes, s0):
            run(self._theta, self._mean_dev, self._sq_mean_dev, self._dev_rows, self._frequency, self._x_dev, self._y_dev,
                idx, sizes, [float(self._lr)] * len(sizes), self._n + s0, losses, slot0=s0)
        return launch

    def _after_resident(self, nb_iterations, losses):
        self._n += nb_iterations
        self._n_cols = min(self._k, -(-self._n // self._frequency))      # hits among counts 0 .. n - 1
        self._loss_dev.copy_(losses[-1].reshape(self._loss_dev.shape))
        self.last_losses = losses.clone()          # (n,) or (n, P); the buffer itself is reused by the next run

    def update_parameters_step(self):
        pass

    def _model_from(self, mean, sq_mean, dev, theta) -> BayesianModel:
        """result()'s model from host moments, the (n_cols, D) deviation rows and weights: a
        MultivariateNormalDiagPlusLowRank per layer."""
        model = BayesianModel(self._model_config)
        for sl, layer_idx in zip(self._spec.layer_slices(), self._weight_layers_indices):
            dist = MultivariateNormalDiagPlusLowRank(mean[sl].copy(), (sq_mean[sl] - mean[sl] ** 2).copy(),
                                                     sqrt(self._scale / (self._k - 1)) * dev[:, sl].T)
            model.apply_distribution(dist, layer_idx, layer_idx)
        model._model.set_flat(theta)
        return model

    def _host_state(self):
        """(mean, sq_mean, dev, theta) on the host with a leading member axis; dev holds the columns filled so far."""
        mean, sq_mean = self._mean_dev.cpu().numpy(), self._sq_mean_dev.cpu().numpy()
        dev, theta = self._dev_rows.cpu().numpy(), self._theta.cpu().numpy()
        if mean.ndim == 1:
            mean, sq_mean, dev, theta = mean[None], sq_mean[None], dev[None], theta[None]
        return mean, sq_mean, dev[:, :self._n_cols], theta

    def member_results(self):
        """One BayesianModel per member of this rank, each built as result() builds its one from that member's rows."""
        mean, sq_mean, dev, theta = self._host_state()
        return [self._model_from(mean[c], sq_mean[c], dev[c], theta[c]) for c in range(self._n_members)]

    def result(self) -> BayesianModel:
        """The posterior model.  With n_members > 1: a Mixture of the members' Gaussians, one distribution over all weight
        layers (see the module docstring); the net's weights are member 0's; this rank's members only."""
        mean, sq_mean, dev, theta = self._host_state()
        if self._n_members == 1:
            return self._model_from(mean[0], sq_mean[0], dev[0], theta[0])
        from ..distributions import Mixture
        components = [MultivariateNormalDiagPlusLowRank(mean[c].copy(), (sq_mean[c] - mean[c] ** 2).copy(),
                                                        sqrt(self._scale / (self._k - 1)) * dev[c].T)
                      for c in range(self._n_members)]
        model = BayesianModel(self._model_config)
        model.apply_distribution(Mixture(components), 0, len(self._net.layers) - 1)
        model._model.set_flat(theta[0])
        return model
