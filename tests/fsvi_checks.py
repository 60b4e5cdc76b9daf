"""Restatement of FSVI.step (Pyesian/optimizers/FSVI.py:60-147, DESIGN assumption A8) for the tests, built on the oracle
without editing it: the forward pass is oracle.mlp's, the draws oracle.philox's, the update oracle.svgd's legacy Adam.
Everything is float64 on the float32 values the device gets, except the assembly of the inputs, which is float32 adds
and is restated bit for bit.  Steps are numbered as in A8."""

from __future__ import annotations

import numpy as np

from oracle import mlp as o_mlp
from oracle import philox as o_philox
from oracle import svgd as o_svgd

F32 = np.float32
STREAM = 9                 # PYZ_STREAM_FSVI
JITTER, REG = 1e-6, 1e-3   # FSVI.py:149 (jitter), :187 (reg)


# ---------------------------------------------------------------- draws (A8 deviation 3)
def draw_xm(seed, t, B, F, lo, hi):
    """X_M (B, F) float32 = lo + u (hi - lo), u from step 4 t (FSVI.py:205), every operation rounded to float32."""
    u = o_philox.uniform(seed, STREAM, 4 * t, B * F).astype(F32).reshape(B, F)
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    return (lo + u * (hi - lo)).astype(F32)


def draw_noise(seed, t, k, F):
    """z (k, F) = 0.1 N(0, 1) from step 4 t + 1 (FSVI.py:87)."""
    return (F32(0.1) * o_philox.normal(seed, STREAM, 4 * t + 1, k * F).astype(F32)).astype(F32).reshape(k, F)


def draw_eps(seed, t, k, D):
    """eps (k, D) from step 4 t + 2 (FSVI.py:231)."""
    return o_philox.normal(seed, STREAM, 4 * t + 2, k * D).astype(F32).reshape(k, D)


# ---------------------------------------------------------------- step 2: inputs
def make_xp(xd, xm, z, shift="prefix"):
    """Xp (k, n, F) float32: batch rows + z_i (FSVI.py:88), then X_M + c_i with c_i = z_0 + ... + z_i summed in float32
    from j = 0 (FSVI.py:89: X_M += noise accumulates over the particle loop).  shift="fresh" is the WRONG variant that
    shifts the measurement rows by z_i alone."""
    xd, xm, z = np.asarray(xd, F32), np.asarray(xm, F32), np.asarray(z, F32)
    out = []
    c = None
    for i in range(len(z)):
        c = z[i].copy() if (c is None or shift == "fresh") else (c + z[i]).astype(F32)
        out.append(np.concatenate([(xd + z[i]).astype(F32), (xm + c).astype(F32)], axis=0))
    return np.stack(out)


# ---------------------------------------------------------------- step 5: GP term
def gram(xp_i):
    """K[r][s] = exp(-|x_r - x_s|^2 / 2) + 1e-6 [r = s] (FSVI.py:151-157), float64 on the float32 inputs."""
    x = np.asarray(xp_i, np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d2) + JITTER * np.eye(len(x))


def gp_alpha(K, f):
    """alpha = K^-1 f: d gp_ll / d f = -alpha (FSVI.py:160-163)."""
    return np.linalg.solve(K, np.asarray(f, np.float64))


# ---------------------------------------------------------------- step 6: Stein term
def stein_system(w):
    """(K_w + 1e-3 I, rhs) of _stein_gradient (FSVI.py:177-195) on the D weights as D scalar points."""
    w = np.asarray(w, np.float64)
    diff = w[:, None] - w[None, :]
    K = np.exp(-0.5 * diff * diff)
    rhs = (-diff * K).sum(axis=1) / len(w)
    return K + REG * np.eye(len(w)), rhs


def stein_c2(w):
    A, rhs = stein_system(w)
    return -np.linalg.solve(A, rhs)


# ---------------------------------------------------------------- step 7: one backward pass
def backprop(theta, x, delta_out, spec):
    """J^T delta: the gradient of sum_r delta_out[r] f[r] with respect to theta, through oracle.mlp's forward."""
    theta = np.asarray(theta, np.float64)
    acts, _ = o_mlp.forward(theta, x, spec)
    ws = o_mlp.unpack(theta, spec)
    delta = np.asarray(delta_out, np.float64).reshape(len(x), 1) * o_mlp._act_grad_from_output(acts[-1], spec.acts[-1])
    grads = [None] * spec.n_layers
    for l in range(spec.n_layers - 1, -1, -1):
        grads[l] = (acts[l].T @ delta, delta.sum(axis=0))
        if l > 0:
            delta = (delta @ ws[l][0].T) * o_mlp._act_grad_from_output(acts[l], spec.acts[l - 1])
    return o_mlp.pack(grads)


def terms(W, xd, y, xm, z, spec, B, shift="prefix", data_scale=None):
    """Steps 2-7 and 9 for the particles W (k, D) on the batch (xd, y): dict(xp, f, alpha, c2, g, loss).
    data_scale: the factor on grad ll_i, k / B as the reference's `1/self._batch_size * self._k` evaluates (FSVI.py:98);
    the tests pass WRONG values to show that they would be caught."""
    W = np.asarray(W, F32)
    k, b = len(W), len(xd)
    y = np.asarray(y, np.float64).reshape(-1)
    scale = (k / B) if data_scale is None else data_scale
    xp = make_xp(xd, xm, z, shift)
    f_all, alpha_all, c2_all = [], [], []
    g = np.zeros(W.shape[1])
    loss = 0.0
    for i in range(k):
        f = o_mlp.predict(W[i], xp[i], spec).reshape(-1)
        alpha = gp_alpha(gram(xp[i]), f)
        c2 = stein_c2(W[i]).astype(F32).astype(np.float64)                  # rounded to float32 once (FSVI.py:115)
        delta = -alpha / k                                                   # (1 / k) J^T (-alpha)
        delta[:b] += scale * (2.0 / b) * (f[:b] - y)                         # (k / B) grad ll_i
        g += backprop(W[i], xp[i], delta, spec) - c2 / k
        loss += ((f[:b] - y) ** 2).mean() / k                               # FSVI.py:123
        f_all.append(f)
        alpha_all.append(alpha)
        c2_all.append(c2)
    return dict(xp=xp, f=np.stack(f_all), alpha=np.stack(alpha_all), c2=np.stack(c2_all), g=g, loss=loss)


# ---------------------------------------------------------------- step 8: update
def adam(mu, g, m, v, t, lr, dtype=np.float64):
    """Keras legacy Adam on mu (FSVI.py:136; Appendix A3)."""
    return o_svgd.adam_update(np.asarray(mu, dtype), np.asarray(g, dtype), np.asarray(m, dtype), np.asarray(v, dtype), int(t),
                              float(lr), dtype)


def adam32(mu, g, m, v, t, lr):
    """The same update in float32 with the device's roundings (k_fsvi_update, as pyz_svgd_gs_adam): 1 - beta evaluated in
    float32 (Keras subtracts float32 tensors), lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t) in float64, rounded once."""
    mu, g, m, v = (np.asarray(a, F32) for a in (mu, g, m, v))
    m = m + (g - m) * (F32(1.0) - F32(0.9))
    v = v + (g * g - v) * (F32(1.0) - F32(0.999))
    lr_t = F32(float(F32(lr)) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
    return mu - lr_t * m / (np.sqrt(v) + F32(1e-7)), m, v


class FsviRef:
    """mu, its Adam slots, the particles and the step counter."""

    def __init__(self, mu0, W0):
        self.mu = np.asarray(mu0, np.float64).copy()
        self.m = np.zeros_like(self.mu)
        self.v = np.zeros_like(self.mu)
        self.W = np.asarray(W0, F32).copy()
        self.t = 0

    def step(self, xd, y, xm, z, eps, spec, B, lr):
        self.t += 1
        out = terms(self.W, xd, y, xm, z, spec, B)
        self.mu, self.m, self.v = adam(self.mu, out["g"], self.m, self.v, self.t, lr)
        self.W = (self.mu[None, :] + np.asarray(eps, np.float64)).astype(F32)   # FSVI.py:228-231
        return out


# ---------------------------------------------------------------- shapes of the device tests
def specs():
    """The three models of the issue: Dense(1) with D = 3, 2 -> 8 -> 1 tanh, 2 -> 8 -> 8 -> 1 relu."""
    return {"dense1": o_mlp.MLPSpec((2, 1), ("linear",), "mse"),
            "tanh8": o_mlp.MLPSpec((2, 8, 1), ("tanh", "linear"), "mse"),
            "relu88": o_mlp.MLPSpec((2, 8, 8, 1), ("relu", "relu", "linear"), "mse")}


def make_problem(spec, rows, B, k, seed):
    """Training rows spread over [-30, 30]^F (so that cond(K_i) stays small: points are far apart on the kernel's
    scale), targets, mu, particles."""
    rng = np.random.default_rng(seed)
    F = spec.dims[0]
    x = rng.uniform(-30.0, 30.0, size=(rows, F)).astype(F32)
    y = rng.normal(size=(rows, 1)).astype(F32)
    mu = (rng.normal(size=spec.n_params) * 0.3).astype(F32)
    W = (mu + rng.normal(size=(k, spec.n_params))).astype(F32)
    return x, y, mu, W


def hard_gp_matrix(n=256):
    """The matrix of deviation 1: n one-dimensional points in [-1, 1] with the 1e-6 jitter, cond ~ 1.9e8."""
    x = np.linspace(-1.0, 1.0, n).astype(F32).reshape(n, 1)
    return gram(x)
