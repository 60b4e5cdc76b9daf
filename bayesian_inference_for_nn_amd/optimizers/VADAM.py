"""VADAM (mirrors Pyesian/optimizers/VADAM.py:15-174; Khan et al. 2018, "Fast and Scalable Bayesian Deep Learning by
Weight-Perturbation in Adam").  Each step perturbs the weights in place, w += eps / sqrt(N (v + lam)) (VADAM.py:59-65,
never undone: the weights random-walk, as in the reference), takes the per-example gradients at the perturbed weights
and applies ADAM's update with m <- b1 m + (1 - b1) (g + lam w / N) and denominator sqrt(v^) + lam / N
(VADAM.py:86-96).  Hyperparameters: lr, beta_1, beta_2, batch_size, optional lam (default 0.5); kwarg starting_model.

Deviations from the reference as written:
  * N is the size of the training split as a float.  VADAM.py:148 takes the int64 tensor train_data.cardinality(),
    which TF will not multiply by float32 tensors without a cast; the port reads it the way BSAM.py:165 does.  The
    `num_data` hyperparameter the reference's drivers pass is ignored by the reference, and here too.
  * lam w / N is computed as (lam / N) w with lam / N rounded to float32 once (the reference rounds lam w, then / N).
  * eps comes from the library's Philox stream (seed, stream 5, step), not TF's global generator.
  * the loss file gets the batch-mean loss of each step (the reference writes the per-example loss vector)."""

from ..distributions import tfd
from ..nn import BayesianModel
from .ADAM import _AdamFamily


class VADAM(_AdamFamily):
    def __init__(self):
        super().__init__()
        self._lam = 0.5

    def compile_extra_components(self, **kwargs):
        self._compile_adam(kwargs)
        if hasattr(self._hyperparameters, "lam"):             # VADAM.py:147
            self._lam = self._hyperparameters.lam
        self._num_data = float(self._training_dataset_cardinality)

    def step(self, save_document_path=None):
        lam_n = float(self._lam) / self._num_data
        perturb = lambda: self._plan.vadam_perturb(self._theta, self._v_dev, self._lam, self._num_data, self._n, self._seed)
        return self._adam_step(save_document_path, lam_n, lam_n, perturb)

    def _launch_run(self, row_idx, losses, sizes, lrs, epochs, s0):
        lam_n = float(self._lam) / self._num_data
        self._plan.adam_run(self._theta, self._m_dev, self._v_dev, self._x_dev, self._y_dev, row_idx, sizes, lrs, epochs,
                            self._beta_1, self._beta_2, losses, denom_eps=lam_n, decay=lam_n, perturb=True, lam=self._lam,
                            num_data=self._num_data, step0=self._n + s0, seed=self._seed, slot0=s0)

    def result(self) -> BayesianModel:
        """Normal(loc = w, scale = v) per Dense layer (VADAM.py:153-172).  As in the reference the scale is the raw
        second-moment vector v, not a standard deviation derived from it."""
        theta, v = self._theta.cpu().numpy(), self._v_dev.cpu().numpy()
        model = self._layer_models(lambda sl: tfd.Normal(theta[sl].copy(), v[sl].copy()))
        model._model.set_flat(theta)
        return model
