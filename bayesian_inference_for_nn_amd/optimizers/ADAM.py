"""ADAM (mirrors Pyesian/optimizers/ADAM.py:13-160): Adam steps from a starting model with the second moment taken
from the batch mean of the SQUARED per-example gradients (the reference squares a tape.jacobian, ADAM.py:60-75), bias
correction by the epoch count; the "posterior" is Deterministic(final weights) per layer.  Hyperparameters: lr,
beta_1, beta_2, batch_size; kwarg starting_model (its weights are copied, ADAM.py:135-136).  One fused device step:
the gradients, their squared means and the update are written by one weight-gradient kernel.

The loss file gets the batch-mean loss of each step, as SGD's does; the reference writes the per-example loss vector
(ADAM.py:57-59)."""

import os

from ..distributions import tfd
from ..distributions.tf import TensorflowProbabilityDistribution
from ..nn import BayesianModel
from .Optimizer import DeviceScalar, Optimizer, fold_running, run_epochs  # noqa: F401  (fold_running: re-exported)


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
        self._count_batch(new_epoch)                           # ADAM.py:46-55: before this step's update
        self._total_batches += 1
        if perturb is not None:
            perturb()
        self._plan.adam_step(self._theta, self._m_dev, self._v_dev, self._x_dev, self._y_dev, self._lr, self._beta_1,
                             self._beta_2, self._epoch_num, self._loss_dev, denom_eps=denom_eps, decay=decay, batch=b,
                             row_idx=idx)
        self._running_dev += self._loss_dev                    # ADAM.py:56
        if save_document_path != None:
            self._append_loss(save_document_path, str(float(self._loss_dev.item())))
        self._n += 1
        return DeviceScalar(self._running_dev.clone(), 0, 1.0 / self._seen_batches)

    # ------------------------------------------------------------------ quiet train(): device-resident runs
    def _launch_run(self, row_idx, losses, sizes, lrs, epochs, s0):
        """Enqueues one chunk of the resident run (steps self._n + s0 ..., loss slots from s0)."""
        raise NotImplementedError

    def _resident_supported(self):
        return os.environ.get("PYZ_ADAM_RUN", "1") != "0" and self._fused_head()

    def _resident_launch(self, nb_iterations):
        """pyz_adam_run / pyz_bsam_run; each chunk's epoch counts follow from _epoch_num and the epochs that the batch
        plans of the run have opened so far."""
        def launch(row_idx, losses, sizes, s0):
            starts = self._plan_epoch_starts             # of this chunk, already among _run_epoch_starts
            before = self._epoch_num + len(self._run_epoch_starts) - len(starts)
            self._launch_run(row_idx, losses, sizes, [float(self._lr)] * len(sizes),
                             run_epochs(before, starts, len(sizes)), s0)
        return launch

    def _after_resident(self, nb_iterations, losses):
        """The bookkeeping of step() for the steps just run (ADAM.py:44-56)."""
        self._total_batches += nb_iterations
        self._count_run(nb_iterations, losses)
        self._loss_dev.copy_(losses[-1].reshape(self._loss_dev.shape))
        self._n += nb_iterations
        self.last_losses = losses.clone()          # the buffer itself is reused by the next run

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
