"""ADAM (mirrors Pyesian/optimizers/ADAM.py:13-160): Adam steps from a starting model with the second moment taken
from the batch mean of the SQUARED per-example gradients (the reference squares a tape.jacobian, ADAM.py:60-75), bias
correction by the epoch count; the "posterior" is Deterministic(final weights) per layer.  Hyperparameters: lr,
beta_1, beta_2, batch_size; kwarg starting_model (its weights are copied, ADAM.py:135-136).  One fused device step:
the gradients, their squared means and the update are written by one weight-gradient kernel.

The loss file gets the batch-mean loss of each step, as SGD's does; the reference writes the per-example loss vector
(ADAM.py:57-59)."""

import os

import numpy as np

from ..distributions import tfd
from ..distributions.tf import TensorflowProbabilityDistribution
from ..nn import BayesianModel
from .Optimizer import DeviceScalar, Optimizer


def run_epochs(epoch_num: int, epoch_starts, n_steps: int):
    """The epoch count each of n_steps consecutive steps uses for its bias correction, as the step loop counts it
    (ADAM.py:49-55: a step that opens a new epoch increments the count BEFORE its update).  epoch_num: the count before
    the first of them; epoch_starts: the steps (0-based) among them that open a new epoch."""
    starts = sorted(int(s) for s in epoch_starts)
    epochs, k = [], 0
    for s in range(int(n_steps)):
        while k < len(starts) and starts[k] <= s:
            k += 1
        epochs.append(int(epoch_num) + k)
    return epochs


def fold_running(running, step_losses, last_epoch_start=None):
    """The epoch's running loss after a run, as the step loop's float32 `running += loss` leaves it (ADAM.py:49-56): summed
    one step after the other, onto the old value -- or from zero at the last step that opened an epoch.  step_losses: (n,)
    the loss of each step, or (n, 2) BSAM's l1, l2, which the step adds as fl(l1 + l2)."""
    a = np.asarray(step_losses, dtype=np.float32)
    if a.ndim == 2:
        a = (a[:, 0] + a[:, 1]).astype(np.float32)
    start = np.float32(running)
    if last_epoch_start is not None:
        start, a = np.float32(0.0), a[int(last_epoch_start):]
    # cumsum is sequential by construction (a pairwise sum would round differently)
    return np.cumsum(np.concatenate([np.asarray([start], dtype=np.float32), a]), dtype=np.float32)[-1]


class _AdamFamily(Optimizer):
    """What ADAM and VADAM share: the moment vectors on the device, the epoch bookkeeping of their step()
    (ADAM.py:44-55, VADAM.py:47-57) and the fused step."""

    def __init__(self):
        super().__init__()
        self._n = None
        self._lr = None
        self._running_loss = 0
        self._seen_batches = 0
        self._total_batches = 0
        self._epoch_num = 1

    def _compile_adam(self, kwargs):
        import torch
        self._lr = self._hyperparameters.lr
        self._batch_size = int(self._hyperparameters.batch_size)
        self._beta_1 = self._hyperparameters.beta_1
        self._beta_2 = self._hyperparameters.beta_2
        start = kwargs["starting_model"]                       # KeyError if absent, like the reference
        self._setup_backend(seed=kwargs.get("seed"))
        self._net.set_weights(start.get_weights())
        self._base_model = self._net
        self._dataset_setup()
        self._theta = torch.as_tensor(self._net.weights_flat.copy()).cuda()
        self._m_dev = torch.zeros(self._D, device="cuda")      # ADAM.py:87-114: zero moments
        self._v_dev = torch.zeros(self._D, device="cuda")
        self._loss_dev = torch.zeros(1, device="cuda")
        self._running_dev = torch.zeros(1, device="cuda")
        self._weight_layers_indices = self._layer_indices()
        self._n = 0

    def _adam_step(self, save_document_path, denom_eps, decay, perturb=None):
        idx, b, new_epoch = self._next_batch()
        self._seen_batches += 1                                # ADAM.py:46-47
        self._total_batches += 1
        if new_epoch:                                          # ADAM.py:49-55: before this step's update
            self._seen_batches = 1
            self._running_dev.zero_()
            self._epoch_num += 1
        if perturb is not None:
            perturb()
        self._plan.adam_step(self._theta, self._m_dev, self._v_dev, self._x_dev, self._y_dev, self._lr, self._beta_1,
                             self._beta_2, self._epoch_num, self._loss_dev, denom_eps=denom_eps, decay=decay, batch=b,
                             row_idx=idx)
        self._running_dev += self._loss_dev                    # ADAM.py:56
        if save_document_path != None:
            with open(save_document_path, "a") as losses_file:
                losses_file.write(str(float(self._loss_dev.item())))
        self._n += 1
        return DeviceScalar(self._running_dev.clone(), 0, 1.0 / self._seen_batches)

    # ------------------------------------------------------------------ quiet train(): device-resident runs
    def _launch_run(self, row_idx, losses, sizes, lrs, epochs, s0):
        """Enqueues one chunk of the resident run (steps self._n + s0 ..., loss slots from s0)."""
        raise NotImplementedError

    _losses_per_step = 1

    def _run_losses(self, n_steps):
        """The persistent loss buffer of the resident runs: _losses_per_step floats per step."""
        return self._res_losses

    def _train_resident(self, nb_iterations: int) -> bool:
        """verbose=False: all steps in device-resident runs (pyz_adam_run / pyz_bsam_run: hipGraph replay, no per-step
        host work), planned chunk by chunk; each chunk's epoch counts follow from _epoch_num and the epochs its batch
        plan opened.  The step loop is taken instead -- decided before anything is enqueued -- for a model the fused step
        does not take, with PYZ_ADAM_RUN=0, or if the library refuses the first chunk; a refusal later is raised."""
        import torch
        from .._lib import PyzError
        if os.environ.get("PYZ_ADAM_RUN", "1") == "0" or self._spec.dims[-1] > 32:
            return False
        if nb_iterations <= 0:
            return True
        # what the batch plan of the first chunk consumes, put back if the library refuses that chunk
        saved = (self._perm_host, self._perm_dev, self._pos, self._epoch, self._rng.bit_generator.state)
        state = {"s0": 0, "last_epoch": None, "epoch_num": self._epoch_num}
        self._reserve_resident(nb_iterations)
        loss_buf = self._run_losses(nb_iterations)

        def launch(row_idx, _losses, sizes, s0):
            starts = list(self._plan_epoch_starts)
            epochs = run_epochs(state["epoch_num"], starts, len(sizes))
            self._launch_run(row_idx, loss_buf, sizes, [float(self._lr)] * len(sizes), epochs, s0)
            state["epoch_num"] = epochs[-1]
            if starts:
                state["last_epoch"] = s0 + starts[-1]
            state["s0"] = s0 + len(sizes)

        try:
            self._run_resident_chunks(nb_iterations, launch)
        except PyzError:
            if state["s0"] > 0:
                raise
            self._perm_host, self._perm_dev, self._pos, self._epoch = saved[:4]
            self._rng.bit_generator.state = saved[4]
            return False
        k = self._losses_per_step
        losses = loss_buf[:k * nb_iterations]
        host = losses.cpu().numpy().reshape(nb_iterations, k)          # (the host has joined the run stream)
        # the bookkeeping of step() for the steps just run (ADAM.py:44-56)
        last_epoch = state["last_epoch"]
        self._total_batches += nb_iterations
        self._seen_batches = self._seen_batches + nb_iterations if last_epoch is None else nb_iterations - last_epoch
        self._epoch_num = state["epoch_num"]
        running = fold_running(float(self._running_dev.item()), host[:, 0] if k == 1 else host, last_epoch)
        self._running_dev.copy_(torch.as_tensor(np.asarray([running], dtype=np.float32)))
        self._loss_dev.copy_(losses[-k:])
        self._n += nb_iterations
        self.last_losses = losses.clone()          # the buffer itself is reused by the next run
        return True

    def _layer_models(self, make_dist):
        model = BayesianModel(self._model_config)
        for sl, layer_idx in zip(self._spec.layer_slices(), self._weight_layers_indices):
            model.apply_distribution(TensorflowProbabilityDistribution(make_dist(sl)), layer_idx, layer_idx)
        return model

    def update_parameters_step(self):
        pass


class ADAM(_AdamFamily):
    def compile_extra_components(self, **kwargs):
        self._compile_adam(kwargs)

    def step(self, save_document_path=None):
        """ADAM.py:42-86: m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) s, w -= lr m^ / (sqrt(v^) + 1e-3)."""
        return self._adam_step(save_document_path, 1e-3, 0.0)

    def _launch_run(self, row_idx, losses, sizes, lrs, epochs, s0):
        self._plan.adam_run(self._theta, self._m_dev, self._v_dev, self._x_dev, self._y_dev, row_idx, sizes, lrs, epochs,
                            self._beta_1, self._beta_2, losses, denom_eps=1e-3, decay=0.0, step0=self._n + s0, slot0=s0)

    def result(self) -> BayesianModel:
        """Deterministic(the layer's current weights) per Dense layer (ADAM.py:142-157)."""
        theta = self._theta.cpu().numpy()
        model = self._layer_models(lambda sl: tfd.Deterministic(theta[sl].copy()))
        model._model.set_flat(theta)
        return model
