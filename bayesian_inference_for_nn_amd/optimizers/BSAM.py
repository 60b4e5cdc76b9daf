"""BSAM (mirrors Pyesian/optimizers/BSAM.py:13-185; Moellenhoff & Khan 2023, "SAM as an Optimal Relaxation of Bayes").
Each step perturbs the weights in place, w += eps / (N v) (BSAM.py:63-68), takes the batch gradient g1 there and ascends,
w += rho g1 / v (BSAM.py:80-92) -- neither is undone, as in the reference -- then takes a second gradient g2 on the same
batch and updates (BSAM.py:103-117)
    m <- b1 m + (1 - b1) (g2 + lam w);  v <- b2 v;  v <- v + (1 - b2) sqrt(v) |g1 + lam + gam|;  w <- w - lr m / v
with the quirks kept as written: the square root of the already scaled v, the FIRST pass's gradient in the v update with
lam and gam added as scalars, no bias correction and no square root in the step's denominator.  m starts at 0 and v at 1
(BSAM.py:121-141).  Hyperparameters: lr, beta_1, beta_2, batch_size, lam, rho, gam (all read unconditionally,
BSAM.py:150-164); kwarg starting_model.  The returned loss is the epoch's running sum of l1 + l2 over the batches seen.
A quiet train() runs as device-resident runs (pyz_bsam_run, see _AdamFamily._train_resident).
One device step is seven launches on the fused path: the perturbation, and for each pass the forward, the head and a
weight-gradient kernel whose epilogue applies the ascent (first pass) or the update (second pass).

Deviations from the reference as written:
  * eps comes from the library's Philox stream (seed, stream 6, step), not TF's global generator.
  * the forward pass whose result is never used (BSAM.py:59) is not executed.
  * lam * w is evaluated in float32 on the device, as are the other products; 1 - beta_1, 1 - beta_2 and 1 / N are
    computed in float64 and rounded to float32 once (the reference's Python-float expressions).
  * the loss file gets the two batch-mean losses of each step, l1 then l2, as the reference writes them."""

from ..distributions import tfd
from ..nn import BayesianModel
from .ADAM import _AdamFamily
from .Optimizer import DeviceScalar


class BSAM(_AdamFamily):
    def __init__(self):
        super().__init__()
        self._lam = 0.5                                        # BSAM.py:44 (compile always overwrites it)

    def compile_extra_components(self, **kwargs):
        import torch
        hyp = self._hyperparameters
        for name in ("lr", "beta_1", "beta_2", "batch_size"):  # BSAM.py:150-153: AttributeError if absent ...
            getattr(hyp, name)
        kwargs["starting_model"]                               # ... then KeyError (BSAM.py:154)
        self._lam = hyp.lam                                    # BSAM.py:162-164: no defaults
        self._rho = hyp.rho
        self._gam = hyp.gam
        self._compile_adam(kwargs)
        self._v_dev.fill_(1.0)                                 # BSAM.py:136: v starts at one
        self._loss_dev = torch.zeros(2, device="cuda")         # l1, l2
        self._num_data = float(self._training_dataset_cardinality)   # BSAM.py:165

    def step(self, save_document_path=None):
        idx, b, new_epoch = self._next_batch()
        self._count_batch(new_epoch)                           # BSAM.py:49-57: before this step's update
        self._total_batches += 1
        self._plan.bsam_step(self._theta, self._m_dev, self._v_dev, self._x_dev, self._y_dev, self._lr, self._beta_1,
                             self._beta_2, self._lam, self._rho, self._gam, self._num_data, self._n, self._seed,
                             self._loss_dev, batch=b, row_idx=idx)
        self._running_dev += self._loss_dev.sum()              # BSAM.py:73,97
        if save_document_path != None:
            l1, l2 = self._loss_dev.tolist()
            self._append_loss(save_document_path, str(l1) + str(l2))
        self._n += 1
        return DeviceScalar(self._running_dev.clone(), 0, 1.0 / self._seen_batches)

    _loss_cols = 2                                             # l1, l2

    def _launch_run(self, row_idx, losses, sizes, lrs, epochs, s0):
        self._plan.bsam_run(self._theta, self._m_dev, self._v_dev, self._x_dev, self._y_dev, row_idx, sizes, lrs,
                            self._beta_1, self._beta_2, self._lam, self._rho, self._gam, self._num_data, self._n + s0,
                            self._seed, losses, slot0=s0)

    def result(self) -> BayesianModel:
        """Normal(loc = w, scale = 1 / (N v)) per Dense layer (BSAM.py:167-182)."""
        theta, v = self._theta.cpu().numpy(), self._v_dev.cpu().numpy()
        scale = (1.0 / (self._num_data * v)).astype(theta.dtype)
        model = self._layer_models(lambda sl: tfd.Normal(theta[sl].copy(), scale[sl].copy()))
        model._model.set_flat(theta)
        return model
