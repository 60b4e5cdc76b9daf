"""Restatement of BSAM.step (Pyesian/optimizers/BSAM.py:46-119) for the tests, built on the oracle without editing it.
The batch-mean loss and its gradient come from oracle.mlp.loss_and_grad; the perturbation, the ascent and the update are
written out in the order the reference applies them, quirks included, with the reference's Python-float scalars
(lr, beta, 1 - beta, lam, rho, gam, 1 / N) rounded to float32 once.  `dtype` is the precision of the state arithmetic:
float64 for the parity tests, float32 to measure how far float32 rounding alone moves a run (the tolerance guard)."""

from __future__ import annotations

import numpy as np

from adam_checks import epoch_plan  # noqa: F401  (the batches of a run: shared with the ADAM tests)
from oracle import mlp as o_mlp

F32 = np.float32

# the two settings of the parity tests: the reference driver's (tests/unittest2.py:133-134) and one at which every
# quirk of the step shows in the result
SETTINGS = {
    "driver": dict(lr=0.5, beta_1=0.9, beta_2=0.9999999, lam=0.0, rho=1e-5, gam=0.1),
    "sharp": dict(lr=0.01, beta_1=0.9, beta_2=0.9, lam=0.5, rho=0.01, gam=0.1),
}


def models():
    """name -> (spec, rows, batch): the six models of the ADAM / VADAM device tests (S = 1 .. 16 waves, gathered rows,
    odd ragged last batches, fused and unfused paths)."""
    from test_gpu_adam_vadam import MODELS
    return MODELS


def make(spec, n, seed=0, scale=0.3):
    """Inputs, labels / targets and starting weights of a model (float32, as the device gets them)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, spec.dims[0])).astype(np.float32)
    if spec.loss == "scce":
        y = rng.integers(0, spec.dims[-1], size=n).astype(np.int32)
    else:
        y = rng.normal(size=(n, spec.dims[-1])).astype(np.float32)
    theta = (rng.normal(size=spec.n_params) * scale).astype(np.float32)
    return x, y, theta


def run_ref(name, setting, steps=21, dtype=np.float64, on_step=None):
    """`steps` restated steps of model `name` at SETTINGS[setting] with injected noise; the batches cross at least three
    epochs.  on_step(i, idx, eps) is called before each step (the device tests run theirs there).
    Returns (restatement, [(l1, l2)])."""
    spec, n, batch = models()[name]
    x, y, theta0 = make(spec, n, seed=sum(map(ord, name)))
    ref = BsamRef(theta0, dtype)
    rng = np.random.default_rng(7)
    plan = epoch_plan(n, batch, steps, seed=3)
    assert len({e for _, e in plan}) >= 3, "the run must cross epochs"
    losses = []
    for i, (idx, _) in enumerate(plan):
        eps = rng.normal(size=spec.n_params).astype(np.float32)
        if on_step is not None:
            on_step(i, idx, eps)
        losses.append(ref.step(x[idx], y[idx], spec, eps, num_data=float(n), **SETTINGS[setting]))
    return ref, losses


def scalars(lr, beta_1, beta_2, lam, rho, gam, num_data):
    """The float32 scalars of one step: every Python-float expression rounded once."""
    return dict(lr=F32(lr), b1=F32(beta_1), c1=F32(1.0 - beta_1), b2=F32(beta_2), c2=F32(1.0 - beta_2), lam=F32(lam),
                rho=F32(rho), gam=F32(gam), inv_n=F32(1.0 / float(num_data)))


class BsamRef:
    """theta, m, v of one chain; m = 0 and v = 1 at the start (BSAM.py:121-141)."""

    def __init__(self, theta0, dtype=np.float64):
        self.dtype = dtype
        self.theta = np.asarray(theta0, dtype=dtype).copy()
        self.m = np.zeros_like(self.theta)
        self.v = np.ones_like(self.theta)
        self.g1 = None

    def _grad(self, x, y, spec):
        loss, g = o_mlp.loss_and_grad(self.theta.astype(np.float64), x, y, spec)[:2]
        return float(loss), np.asarray(g).astype(self.dtype)

    def step(self, x, y, spec, eps, lr, beta_1, beta_2, lam, rho, gam, num_data):
        """One BSAM.step on the batch (x, y) with the injected standard normals eps; returns (l1, l2)."""
        c = {k: self.dtype(v) for k, v in scalars(lr, beta_1, beta_2, lam, rho, gam, num_data).items()}
        self.theta = self.theta + np.asarray(eps, dtype=self.dtype) * (c["inv_n"] / self.v)      # :63-68, never undone
        l1, g1 = self._grad(x, y, spec)                                                          # :70-78
        self.theta = self.theta + c["rho"] * (g1 / self.v)                                       # :80-92, never undone
        self.g1 = g1
        l2, g2 = self._grad(x, y, spec)                                                          # :94-101
        self.m = c["b1"] * self.m + c["c1"] * (g2 + c["lam"] * self.theta)                       # :110-111
        self.v = c["b2"] * self.v                                                                # :113
        self.v = self.v + c["c2"] * (np.sqrt(self.v) * np.abs(g1 + c["lam"] + c["gam"]))         # :114-115
        self.theta = self.theta - c["lr"] * self.m / self.v                                      # :117
        return l1, l2
