"""Restatement of ADAM.step / VADAM.step (Pyesian/optimizers/ADAM.py:42-86, VADAM.py:44-98) for the tests, built on
the oracle without editing it.  The per-example gradients come LITERALLY from oracle.mlp.loss_and_grad called on single
rows (the reference's tape.jacobian of the unreduced loss), their mean and mean square are taken in float64, and the
updates apply the reference's scalars rounded to float32 once (TF turns each Python-float expression -- 1 - beta,
1 - beta^epoch, lam / N, lr -- into one float32 tensor).  None of this uses the (A o A)^T (Delta o Delta) identity the
kernels rely on, so a parity check against it tests that identity."""

from __future__ import annotations

import numpy as np

from oracle import mlp as o_mlp

F32 = np.float32


def per_example_grads(theta, x, y, spec):
    """(B, D) float64: row i = gradient of example i's own loss."""
    return np.stack([o_mlp.loss_and_grad(theta, x[i:i + 1], y[i:i + 1], spec)[1] for i in range(len(x))])


def grad_moments(theta, x, y, spec):
    """(batch-mean loss, g = mean_i g_i, s = mean_i g_i^2), float64; rows are taken one at a time (no (B, D) matrix)."""
    loss, _, _ = o_mlp.loss_and_grad(theta, x, y, spec)
    g = np.zeros(spec.n_params)
    s = np.zeros(spec.n_params)
    for i in range(len(x)):
        gi = o_mlp.loss_and_grad(theta, x[i:i + 1], y[i:i + 1], spec)[1]
        g += gi
        s += gi * gi
    return float(loss), g / len(x), s / len(x)


def identity_moments(theta, x, y, spec):
    """(g, s) through the identity the kernels use, in float64: per layer, g = A^T Delta and
    s = (A o A)^T ((B Delta) o (B Delta)) / B with A = [input, 1] and Delta = d (mean loss) / d pre-activation."""
    acts, _ = o_mlp.forward(theta, x, spec)
    out = acts[-1]
    B = len(x)
    if spec.loss == "scce":
        delta = out.copy()
        delta[np.arange(B), np.asarray(y).reshape(-1).astype(np.int64)] -= 1.0
        delta /= B
    else:
        delta = 2.0 * (out - np.asarray(y, dtype=np.float64).reshape(out.shape)) / (B * out.shape[1])
        delta = delta * o_mlp._act_grad_from_output(out, spec.acts[-1])
    ws = o_mlp.unpack(np.asarray(theta, dtype=np.float64), spec)
    gs, ss = [None] * spec.n_layers, [None] * spec.n_layers
    for l in range(spec.n_layers - 1, -1, -1):
        a = np.concatenate([acts[l], np.ones((B, 1))], axis=1)
        gs[l] = (a.T @ delta).reshape(-1)
        ss[l] = ((a * a).T @ ((B * delta) ** 2)).reshape(-1) / B
        if l > 0:
            delta = (delta @ ws[l][0].T) * o_mlp._act_grad_from_output(acts[l], spec.acts[l - 1])
    return np.concatenate(gs), np.concatenate(ss)


def scalars(lr, beta_1, beta_2, epoch, denom_eps=1e-3, decay=0.0):
    """The float32 scalars of one update: every Python-float expression rounded once."""
    return dict(lr=F32(lr), b1=F32(beta_1), c1=F32(1.0 - beta_1), b2=F32(beta_2), c2=F32(1.0 - beta_2),
                bc1=F32(1.0 - beta_1 ** epoch), bc2=F32(1.0 - beta_2 ** epoch), eps=F32(denom_eps), decay=F32(decay))


class AdamRef:
    """theta, m, v of one chain (float64 arithmetic, float32 scalars)."""

    def __init__(self, theta0):
        self.theta = np.asarray(theta0, dtype=np.float64).copy()
        self.m = np.zeros_like(self.theta)
        self.v = np.zeros_like(self.theta)

    def perturb(self, eps, lam, num_data):
        """VADAM.py:59-65: w += eps / sqrt(N (v + lam)) (not undone)."""
        self.theta = self.theta + eps / np.sqrt(np.float64(F32(num_data)) * (self.v + np.float64(F32(lam))))

    def step(self, x, y, spec, lr, beta_1, beta_2, epoch, denom_eps=1e-3, decay=0.0):
        """One ADAM.step update (ADAM.py:60-84) -- VADAM.py:86-96 with decay = denom_eps = lam / N; returns the batch loss."""
        loss, g, s = grad_moments(self.theta, x, y, spec)
        c = {k: np.float64(v) for k, v in scalars(lr, beta_1, beta_2, epoch, denom_eps, decay).items()}
        self.m = c["b1"] * self.m + c["c1"] * (g + c["decay"] * self.theta)
        self.v = c["b2"] * self.v + c["c2"] * s
        mh, vh = self.m / c["bc1"], self.v / c["bc2"]
        self.theta = self.theta - c["lr"] * mh / (np.sqrt(vh) + c["eps"])
        return loss


def epoch_plan(n_rows, batch, n_steps, seed):
    """(row indices, epoch number) of n_steps consecutive batches: a fresh permutation per epoch, ragged last batch;
    the epoch count starts at 1 and advances with the first batch of a new epoch (ADAM.py:49-55)."""
    rng = np.random.default_rng(seed)
    out, epoch = [], 0
    while len(out) < n_steps:
        epoch += 1
        perm = rng.permutation(n_rows).astype(np.int32)
        for o in range(0, n_rows, batch):
            if len(out) < n_steps:
                out.append((perm[o:o + batch], epoch))
    return out
