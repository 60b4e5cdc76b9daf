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
        import torch
        self._n_members = _members.n_members_of(kwargs)
        if self._n_members > 1:
            return self._compile_members(**kwargs)
        self._frequency = self._hyperparameters.frequency
        self._lr = self._hyperparameters.lr
        self._batch_size = self._hyperparameters.batch_size
        self._setup_backend(seed=kwargs.get("seed"))
        start = kwargs["starting_model"]                       # KeyError if absent, like the reference
        self._net.set_weights(start.get_weights())
        self._base_model = self._net
        self._dataset_setup()
        self._theta = torch.as_tensor(self._net.weights_flat.copy()).cuda()
        self._mean_dev = self._theta.clone()                   # SGD.py:100-107: the "mean" starts as the weights
        self._loss_dev = torch.zeros(1, device="cuda")
        self._running_dev = torch.zeros(1, device="cuda")
        self._weight_layers_indices = self._layer_indices()
        self._n = 0

    def _compile_members(self, **kwargs):
        """n_members = P > 1: a plan for P particles and a (P, D) state (see the module docstring for the starts)."""
        import torch
        P = self._n_members
        self._frequency = self._hyperparameters.frequency
        self._lr = self._hyperparameters.lr
        self._batch_size = self._hyperparameters.batch_size
        start = kwargs["starting_model"]                       # KeyError if absent, like the reference
        _members.check_starts(start, P)
        self._setup_backend(seed=kwargs.get("seed"), max_particles=P, chains_per_rank=P)
        self._theta = torch.as_tensor(_members.member_starts(self, start, P)).cuda()
        self._base_model = self._net
        self._dataset_setup()
        self._mean_dev = self._theta.clone()                   # SGD.py:100-107: the "mean" starts as the weights
        self._loss_dev = torch.zeros(P, device="cuda")
        self._running_dev = torch.zeros(1, device="cuda")
        self._weight_layers_indices = self._layer_indices()
        self._n = 0

    def _reserve_resident(self, n_steps: int):
        if self._n_members == 1:
            return super()._reserve_resident(n_steps)
        _members.reserve_resident(self, n_steps, self._n_members)

    def _step_members(self, save_document_path=None):
        idx, b, new_epoch = self._next_batch()
        self._seen_batches += 1
        if new_epoch:
            self._seen_batches = 1
            self._running_dev.zero_()
            self._epoch_num += 1
        self._plan.sgd_members_step(self._theta, self._mean_dev, self._x_dev, self._y_dev, self._lr, self._n,
                                    self._n % self._frequency == 0, self._loss_dev, batch=b, row_idx=idx)
        self._running_dev += self._loss_dev.mean()             # the mean over members of the batch loss
        if save_document_path != None:
            with open(save_document_path, "a") as losses_file:
                losses_file.write(str(float(self._loss_dev.mean().item())))
        self._n += 1
        return DeviceScalar(self._running_dev.clone(), 0, 1.0 / self._seen_batches)

    def _train_resident_members(self, nb_iterations: int) -> bool:
        """verbose=False: all steps in one members run.  The kernel keeps the "mean" on the hit steps itself, so the run
        is not cut at the last hit as the one-member run is; the epoch bookkeeping is step()'s."""
        if nb_iterations <= 0:
            return True
        epoch_starts = []

        def launch(idx, loss_buf, sizes, s0):
            epoch_starts.extend(s0 + e for e in self._plan_epoch_starts)      # of the chunk just planned
            self._plan.sgd_members_run(self._theta, self._mean_dev, self._frequency, self._x_dev, self._y_dev, idx, sizes,
                                       [float(self._lr)] * len(sizes), self._n + s0, loss_buf, slot0=s0)
        losses = self._run_resident_chunks(nb_iterations, launch)
        per_step = losses.mean(dim=1)
        if not epoch_starts:
            self._seen_batches += nb_iterations
            self._running_dev += per_step.sum()
        else:
            self._epoch_num += len(epoch_starts)
            self._seen_batches = nb_iterations - epoch_starts[-1]
            self._running_dev.copy_(per_step[epoch_starts[-1]:].sum().reshape(1))
        self._loss_dev.copy_(losses[-1])
        self._n += nb_iterations
        self.last_losses = losses.clone()          # (n, P); the buffer itself is reused by the next run
        return True

    def step(self, save_document_path=None):
        if self._n_members > 1:
            return self._step_members(save_document_path)
        idx, b, new_epoch = self._next_batch()
        self._seen_batches += 1                                # SGD.py:45
        if new_epoch:                                          # SGD.py:48-54
            self._seen_batches = 1
            self._running_dev.zero_()
            self._epoch_num += 1
        self._plan.sgd_step(self._theta, self._x_dev, self._y_dev, self._lr, self._loss_dev, batch=b, row_idx=idx)
        self._running_dev += self._loss_dev                    # SGD.py:60
        if save_document_path != None:
            with open(save_document_path, "a") as losses_file:
                losses_file.write(str(float(self._loss_dev.item())))
        if self._n % self._frequency == 0:                     # SGD.py:78-84: mean <- theta
            self._mean_dev.copy_(self._theta)
        self._n += 1
        return DeviceScalar(self._running_dev.clone(), 0, 1.0 / self._seen_batches)

    def _train_resident(self, nb_iterations: int) -> bool:
        """verbose=False: all steps in device-resident runs (hipGraph replay, no per-step host work).  The
        "mean" of SGD.py:78-84 is the weights after the last step whose count is a multiple of `frequency`:
        the run is cut there, the weights copied, and the rest follows."""
        import torch
        from .._lib import PyzError
        if self._n_members > 1:
            return self._train_resident_members(nb_iterations)
        if nb_iterations <= 0:
            return True
        table, sizes = self._batch_plan(nb_iterations)
        idx, loss_buf = self._resident_buffers(table, nb_iterations)
        losses = loss_buf[:nb_iterations]
        lrs = [float(self._lr)] * nb_iterations
        freq = int(self._frequency)
        hits = [s for s in range(nb_iterations) if (self._n + s) % freq == 0]
        cut = hits[-1] + 1 if hits else 0             # steps [0, cut) end with the last "mean <- weights"
        stream = self._run_stream()
        stream.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(stream):
                if cut > 0:
                    self._plan.sgd_run(self._theta, self._x_dev, self._y_dev, idx, sizes[:cut], lrs[:cut], losses)
                    self._mean_dev.copy_(self._theta)
                if cut < nb_iterations:
                    self._plan.sgd_run(self._theta, self._x_dev, self._y_dev, idx, sizes[cut:], lrs[cut:], losses, slot0=cut)
        except PyzError:                              # shapes the fused step does not take: per-step loop
            if cut > 0:
                raise
            return False
        self._join_run(stream)
        self._warn_if_diverged(stream)
        # epoch bookkeeping of step() (SGD.py:45-60) for the steps just run
        last_epoch = self._plan_epoch_starts[-1] if self._plan_epoch_starts else None
        if last_epoch is None:
            self._seen_batches += nb_iterations
            self._running_dev += losses.sum()
        else:
            self._epoch_num += len(self._plan_epoch_starts)
            self._seen_batches = nb_iterations - last_epoch
            self._running_dev.copy_(losses[last_epoch:].sum().reshape(1))
        self._loss_dev.copy_(losses[-1:])
        self._n += nb_iterations
        self.last_losses = losses.clone()          # the buffer itself is reused by the next run
        return True

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
