"""Plain mini-batch SGD; the "posterior" is Deterministic(last weights) per layer
(mirrors Pyesian/optimizers/SGD.py:13-149).  Hyperparameters: lr, frequency, batch_size;
kwarg starting_model (its weights are copied, SGD.py:121-122).

Extension: kwarg n_members = P > 1 trains P models -- a deep ensemble -- in one particle-batched step (the reference
trains one; n_members absent or 1 is that path, untouched).  starting_model may be a list of P models (member c copies
entry c) or one model (member 0 copies it, member c >= 1 starts from the Glorot draw of seed + c).  All members of a
rank see the rank's minibatches, like SGLD's chains: the diversity comes from the starts.  member_results() gives one
BayesianModel per member, member_models() the P networks (what a MultiSWAG run starts from), result() one model whose
single distribution over ALL weight layers is Sampled(the P "mean" rows, equal frequencies) -- a draw takes every
layer from the same member --, with member 0's weights in the net.  With several ranks result() is the rank's own:
members are not merged across ranks."""

import numpy as np

from ..distributions import tfd
from ..distributions.tf import TensorflowProbabilityDistribution
from ..nn import BayesianModel
from . import _members
from .Optimizer import DeviceScalar, Optimizer


class SGD(Optimizer):
    _conv_models = True      # a model with Conv2D layers trains through step(), one member

    def __init__(self):
        super().__init__()
        self._n = None
        self._lr = None
        self._frequency = None
        self._k = None
        self._running_loss = 0
        self._seen_batches = 0
        self._epoch_num = 1
        self._n_members = 1

    def compile_extra_components(self, **kwargs):
        """A plan for P = n_members particles; the state is (D,) for one member, the reference's path, and (P, D) for
        several (see the module docstring for the starts)."""
        import torch
        P = self._n_members = _members.n_members_of(kwargs)
        self._frequency = self._hyperparameters.frequency
        self._lr = self._hyperparameters.lr
        self._batch_size = self._hyperparameters.batch_size
        start = kwargs["starting_model"]                       # KeyError if absent, like the reference
        _members.check_starts(start, P)
        self._setup_backend(seed=kwargs.get("seed"), max_particles=P, chains_per_rank=P)
        rows = _members.member_starts(self, start, P)          # SGD.py:121-122: the starting model's weights are copied
        self._theta = torch.as_tensor(rows if P > 1 else rows[0]).cuda()
        self._base_model = self._net
        self._dataset_setup()
        self._mean_dev = self._theta.clone()                   # SGD.py:100-107: the "mean" starts as the weights
        self._loss_dev = torch.zeros(P, device="cuda")
        self._running_dev = torch.zeros(1, device="cuda")
        self._weight_layers_indices = self._layer_indices()
        self._n = 0
        if P > 1:
            self._loss_cols = P                                # a loss per member and step
        else:
            self._resident_chunks = self._ONE_CHUNK            # the one-member run is planned in one piece

    def step(self, save_document_path=None):
        idx, b, new_epoch = self._next_batch()
        self._count_batch(new_epoch)                           # SGD.py:45-54
        hit = self._n % self._frequency == 0                   # SGD.py:78-84: mean <- theta
        if self._n_members > 1:
            self._plan.sgd_members_step(self._theta, self._mean_dev, self._x_dev, self._y_dev, self._lr, self._n, hit,
                                        self._loss_dev, batch=b, row_idx=idx)
            loss = self._loss_dev.mean()                       # the mean over members of the batch loss
        else:
            self._plan.sgd_step(self._theta, self._x_dev, self._y_dev, self._lr, self._loss_dev, batch=b, row_idx=idx)
            loss = self._loss_dev
            if hit:
                self._mean_dev.copy_(self._theta)
        self._running_dev += loss                              # SGD.py:60
        if save_document_path != None:
            self._append_loss(save_document_path, str(float(loss.item())))
        self._n += 1
        return DeviceScalar(self._running_dev.clone(), 0, 1.0 / self._seen_batches)

    # ------------------------------------------------------------------ quiet train(): device-resident runs
    def _resident_supported(self):
        return not self._conv and (self._n_members > 1 or self._fused_head())

    def _resident_launch(self, nb_iterations):
        lr, freq = float(self._lr), int(self._frequency)
        if self._n_members > 1:
            # the members kernel keeps the "mean" on the hit steps itself: no cut
            def launch(idx, losses, sizes, s0):
                self._plan.sgd_members_run(self._theta, self._mean_dev, freq, self._x_dev, self._y_dev, idx, sizes,
                                           [lr] * len(sizes), self._n + s0, losses, slot0=s0)
            return launch

        def launch(idx, losses, sizes, s0):
            """The "mean" of SGD.py:78-84 is the weights after the last step whose count is a multiple of `frequency`:
            the run is cut there, the weights copied, and the rest follows."""
            n, n0 = len(sizes), self._n + s0
            lrs = [lr] * n
            cut = max(0, (n0 + n - 1) // freq * freq - n0 + 1)    # steps [0, cut) end with the last "mean <- weights"
            if cut > 0:
                self._plan.sgd_run(self._theta, self._x_dev, self._y_dev, idx, sizes[:cut], lrs[:cut], losses, slot0=s0)
                self._mean_dev.copy_(self._theta)
            if cut < n:
                self._plan.sgd_run(self._theta, self._x_dev, self._y_dev, idx, sizes[cut:], lrs[cut:], losses,
                                   slot0=s0 + cut)
        return launch

    def _after_resident(self, nb_iterations, losses):
        """The bookkeeping of step() (SGD.py:45-60) for the steps just run."""
        self._count_run(nb_iterations, losses.mean(dim=1) if self._n_members > 1 else losses)
        self._loss_dev.copy_(losses[-1].reshape(self._loss_dev.shape))
        self._n += nb_iterations
        self.last_losses = losses.clone()          # (n,) or (n, P); the buffer itself is reused by the next run

    def _model_from(self, mean, theta) -> BayesianModel:
        """result()'s model from a host "mean" vector and weights: Deterministic(mean) per layer."""
        model = BayesianModel(self._model_config)
        for sl, layer_idx in zip(self._spec.layer_slices(), self._weight_layers_indices):
            dist = TensorflowProbabilityDistribution(tfd.Deterministic(mean[sl].copy()))
            model.apply_distribution(dist, layer_idx, layer_idx)
        model._model.set_flat(theta)
        return model

    def member_results(self):
        """One BayesianModel per member of this rank, each built as result() builds its one from that member's row."""
        mean, theta = self._mean_dev.cpu().numpy(), self._theta.cpu().numpy()
        if mean.ndim == 1:
            mean, theta = mean[None, :], theta[None, :]
        return [self._model_from(mean[c], theta[c]) for c in range(self._n_members)]

    def member_models(self):
        """The members' networks: P DenseNets with the members' current weights."""
        from ..nn.model import model_from_json
        theta = self._theta.cpu().numpy()
        if theta.ndim == 1:
            theta = theta[None, :]
        models = []
        for c in range(self._n_members):
            net = model_from_json(self._model_config)
            net.set_flat(theta[c])
            models.append(net)
        return models

    def result(self) -> BayesianModel:
        """The posterior model.  With n_members > 1: Sampled over the members' "mean" rows, one distribution over all
        weight layers (a draw is one member, every layer of it); the net's weights are member 0's; this rank's members
        only."""
        mean, theta = self._mean_dev.cpu().numpy(), self._theta.cpu().numpy()
        if self._n_members == 1:
            return self._model_from(mean, theta)
        from ..distributions import Sampled
        model = BayesianModel(self._model_config)
        P = self._n_members
        model.apply_distribution(Sampled([mean[c].copy() for c in range(P)], [1] * P), 0, len(self._net.layers) - 1)
        model._model.set_flat(theta[0])
        return model

    def update_parameters_step(self):
        pass
