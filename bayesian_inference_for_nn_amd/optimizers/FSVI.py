"""FSVI (mirrors Pyesian/optimizers/FSVI.py:34-290; Rudner et al., "Tractable Function-Space Variational Inference in
Bayesian Neural Networks", arXiv 2312.17199).  A mean-field posterior N(mu, 1) over the D weights is fitted through k
particles W_i = mu + eps_i.  Each step (FSVI.py:60-147, DESIGN assumption A8) draws B measurement points uniformly in the
bounding box of the training inputs, shifts batch and measurement points by per-particle input noise -- the measurement
points by the running sum of the noises, as the reference's X_M += noise does -- and sums over the particles
    (k / B) grad ll_i  -  (1 / k) J_i^T alpha_i  -  (1 / k) c2_i
with ll_i the batch-mean squared error, alpha_i = (K_i + 1e-6 I)^-1 f_i the gradient of a zero-mean GP prior with an RBF
kernel over the batch and measurement points, and c2_i a Stein score estimate over the D weights taken as D scalar points.
Keras legacy Adam applies the sum to mu (only optimizers[0] is used, FSVI.py:136), then every particle is redrawn around
the new mu (FSVI.py:228-231).  The returned loss is sum_i ll_i / k.  Hyperparameters: batch_size, lr, k; kwargs prior and
function_prior (both read unconditionally, FSVI.py:272,277), seed.  Both solves run on the device in float64
(pyz_spd_solve_f64); the method needs the MeanSquaredError loss, a last layer of one unit, batch_size + batch rows <= 1024
and D <= 2048 weights (the Stein system is D x D).

Deviations from the reference as written:
  * the GP solve is float64, not float32: 256 one-dimensional points in [-1, 1] give cond(K) = 1.9e8 with the 1e-6 jitter.
  * mu starts at the prior's flat mean and the particles are drawn from the prior on the device, as SVGD's are; the
    reference's _posterior_means list (FSVI.py:242) only has the right length for D = 2.
  * every draw comes from the library's Philox stream 9 of the seed -- step 4 t the measurement set, 4 t + 1 the input
    noise, 4 t + 2 the redraw (row i is elements [i D, (i + 1) D)), step 0 the initial particles -- not from TF's and
    NumPy's global generators.
  * the plot of step 250 (a NameError in the reference), the per-step print and visualize_data are not carried.
  * a Cholesky pivot that is not positive makes that step's loss NaN and counts in the plan's non-finite sentinel;
    nothing is masked.
  * result() returns an Ensemble (the list SVGD returns, with the ensemble-mean predict) of the k particle models, the
    reference a plain list (FSVI.py:285-290); posterior() is the BayesianModel with Normal(mu, 1) per layer."""

import numpy as np

from ..distributions import tfd
from ..distributions.tf import TensorflowProbabilityDistribution
from ..nn import BayesianModel
from ..nn.model import model_from_json
from .Optimizer import DeviceScalar, Optimizer
from .SVGD import Ensemble


class FSVI(Optimizer):
    def __init__(self):
        super().__init__()
        self._step = 0
        self._k = None
        self._prior = None

    def compile_extra_components(self, **kwargs):
        import torch
        from .. import _lib
        from ..engine import MLPPlan, fill_normal
        self._batch_size = int(self._hyperparameters.batch_size)      # FSVI.py:268
        self._k = int(self._hyperparameters.k)                        # FSVI.py:270
        self._prior = kwargs["prior"]                                 # FSVI.py:272: KeyError if absent
        self._lr = self._hyperparameters.lr                           # FSVI.py:274
        self._function_prior = kwargs["function_prior"]               # FSVI.py:277: KeyError if absent ("GP": the RBF prior)
        self._setup_backend(seed=kwargs.get("seed"), max_particles=max(self._k, 1))
        # the step forwards batch + measurement rows of every particle at once: a plan of that many rows
        self._plan.close()
        self._plan = MLPPlan(self._spec, max_batch=2 * self._batch_size, max_particles=max(self._k, 1))
        self._base_model = self._net
        self._dataset_setup()
        self._weight_layers_indices = self._layer_indices()
        # FSVI.py:199-201 recomputes the bounding box of the training inputs every step, to the same values
        self._lo = self._x_dev.min(dim=0).values.contiguous()
        self._hi = self._x_dev.max(dim=0).values.contiguous()
        # _init_weights (FSVI.py:233-245): a prior sample per particle; mu = the prior's mean
        mu, rho = self._prior.flat(self._net)
        self._mu = torch.as_tensor(np.ascontiguousarray(mu, dtype=np.float32)).cuda()
        w = torch.empty((max(self._k, 1), self._D), device="cuda")
        fill_normal(w, self._seed, _lib.STREAM_FSVI, 0, 0.0, 1.0)
        self._weights = (w * torch.as_tensor(np.asarray(rho, dtype=np.float32)).cuda() + self._mu).contiguous()[:self._k]
        self._adam_m = torch.zeros(self._D, device="cuda")
        self._adam_v = torch.zeros(self._D, device="cuda")
        self._loss_dev = torch.zeros(1, device="cuda")

    def step(self, save_document_path=None):
        self._step += 1                                               # FSVI.py:61
        idx, b, _ = self._next_batch()
        self._plan.fsvi_step(self._mu, self._weights, self._adam_m, self._adam_v, self._x_dev, self._y_dev,
                             self._batch_size, self._lr, self._step, self._seed, self._loss_dev, lo=self._lo, hi=self._hi,
                             batch=b, row_idx=idx)
        return DeviceScalar(self._loss_dev.clone(), 0)                # FSVI.py:147

    def update_parameters_step(self):
        pass

    def result(self):
        """The k particle models (FSVI.py:285-290)."""
        W = self._weights.cpu().numpy()
        ensemble = Ensemble()
        for i in range(self._k):
            m = model_from_json(self._model_config)
            m.set_flat(W[i])
            ensemble.append(m)
        return ensemble

    def posterior(self) -> BayesianModel:
        """Normal(mu, 1) per Dense layer: what FSVI.py:228-231 draws the particles from."""
        mu = self._mu.cpu().numpy()
        model = BayesianModel(self._model_config)
        for sl, layer_idx in zip(self._spec.layer_slices(), self._weight_layers_indices):
            dist = TensorflowProbabilityDistribution(tfd.Normal(mu[sl].copy(), np.ones_like(mu[sl])))
            model.apply_distribution(dist, layer_idx, layer_idx)
        model._model.set_flat(mu)
        return model
