"""Float64 restatement of the Deep-PILCO policy update (Pyesian/dynamics/deep_pilco.py:247-326) for the tests of
pyz_pilco_policy_step: the particle rollout, its cost, the cost's gradient by torch CPU autograd, the Keras-Adam step,
and the table of cases.  Nothing here touches the library under test.

  for t = 1..H, s = s_{t-1}:  a_i = policy(phi, s_i)   (the output itself: softmax probabilities)
                              y_i = dynamics(W_i, [s_i, a_i])
                              m = mean_i y_i, sd = sqrt(mean_i (y_i - m)^2)  (tf.math.reduce_std), s_t,i = m + sd eps[t-1, i]
  cost = -mean_i r(s_0,i, 0); at each t with t % freq == 0: discount *= gamma, then cost -= discount mean_i r(s_t,i, t)
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

GAMMA = 0.95
REWARD_MIN_S = {"Cart": 4, "Acb 2 factors": 5}


def default_freq(H: int) -> int:
    return max(int(H / 25), 1)


@dataclass(frozen=True)
class Case:
    name: str
    S: int
    A: int
    K: int
    H: int
    pol_hidden: Tuple[int, ...]
    pol_hidden_act: str
    pol_out: str
    dyn_hidden: Tuple[int, ...]
    dyn_hidden_act: str
    reward: str

    @property
    def pol_dims(self):
        return (self.S,) + self.pol_hidden + (self.A,)

    @property
    def pol_acts(self):
        return (self.pol_hidden_act,) * len(self.pol_hidden) + (self.pol_out,)

    @property
    def dyn_dims(self):
        return (self.S + self.A,) + self.dyn_hidden + (self.S,)

    @property
    def dyn_acts(self):
        return (self.dyn_hidden_act,) * len(self.dyn_hidden) + ("linear",)

    @property
    def freq(self):
        return default_freq(self.H)


CASES = [
    Case("min", 4, 1, 2, 1, (), "relu", "relu", (7,), "relu", "Cart"),
    Case("cart_softmax", 4, 2, 5, 8, (8,), "tanh", "softmax", (16,), "relu", "Cart"),
    Case("acb_two_hidden", 6, 3, 7, 12, (10,), "relu", "softmax", (24, 12), "relu", "Acb 2 factors"),
    Case("freq2", 4, 2, 3, 50, (8,), "relu", "softmax", (16,), "relu", "Cart"),
    Case("odd", 6, 3, 33, 26, (33,), "relu", "softmax", (65,), "relu", "Acb 2 factors"),
    Case("box_linear", 4, 1, 32, 32, (16,), "relu", "linear", (64, 32), "tanh", "Cart"),
    Case("sigmoid", 4, 2, 5, 8, (8,), "sigmoid", "softmax", (16,), "sigmoid", "Cart"),
    Case("example", 6, 3, 32, 32, (80,), "tanh", "softmax", (512, 256), "relu", "Acb 2 factors"),
]
CASE = {c.name: c for c in CASES}
# the seed of a case's inputs.  `min` has a single relu output unit: with seed 0 it is dead for both particles and the
# gradient is identically zero, which would check nothing (test_pilco_host asserts a non-zero gradient for every case)
SEED = {"min": 1}


def n_params(dims):
    return sum((i + 1) * o for i, o in zip(dims[:-1], dims[1:]))


def draw_flat(rng, dims, gain):
    """Flat layout (kernel (in, out) row-major, then bias, per layer): kernels N(0, gain^2 / fan_in), biases N(0, 0.1^2)."""
    parts = []
    for i, o in zip(dims[:-1], dims[1:]):
        parts.append(rng.normal(size=(i, o)).ravel() * gain / np.sqrt(i))
        parts.append(rng.normal(size=o) * 0.1)
    return np.concatenate(parts)


def make_inputs(case: Case, seed=None):
    """float64 inputs of a case: phi (D_pol,), W (K, D_dyn), s0 (K, S) uniform in +-0.05, eps (H, K, S) unit normals."""
    seed = SEED.get(case.name, 0) if seed is None else seed
    rng = np.random.default_rng([seed, CASES.index(case)])
    phi = draw_flat(rng, case.pol_dims, 1.0)
    W = np.stack([draw_flat(rng, case.dyn_dims, 0.7) for _ in range(case.K)])
    s0 = rng.uniform(-0.05, 0.05, size=(case.K, case.S))
    eps = rng.normal(size=(case.H, case.K, case.S))
    return dict(phi=phi, W=W, s0=s0, eps=eps)


def _act(z, name):
    if name == "relu":
        return torch.relu(z)
    if name == "tanh":
        return torch.tanh(z)
    if name == "sigmoid":
        return torch.sigmoid(z)
    if name == "softmax":
        return torch.softmax(z, dim=-1)
    assert name == "linear", name
    return z


def _mlp_shared(theta, dims, acts, x):
    """x (K, in) through one parameter vector."""
    off = 0
    for (i, o), a in zip(zip(dims[:-1], dims[1:]), acts):
        w = theta[off:off + i * o].reshape(i, o)
        b = theta[off + i * o:off + (i + 1) * o]
        off += (i + 1) * o
        x = _act(x @ w + b, a)
    return x


def _mlp_per_row(thetas, dims, acts, x):
    """row i of x (K, in) through row i of thetas (K, D)."""
    off = 0
    for (i, o), a in zip(zip(dims[:-1], dims[1:]), acts):
        w = thetas[:, off:off + i * o].reshape(-1, i, o)
        b = thetas[:, off + i * o:off + (i + 1) * o]
        off += (i + 1) * o
        x = _act(torch.einsum("ki,kio->ko", x, w) + b, a)
    return x


def reward(name, s, t):
    """r(s, t) of dynamics/custom.py:6-18 on the last axis of s (tensor or array)."""
    if name == "Cart":
        return -s[..., 2] - s[..., 3] * s[..., 2] + t * (-s[..., 2] ** 2 + 0.2095 ** 2)
    assert name == "Acb 2 factors", name
    return 4 - 3 * s[..., 0] - (s[..., 0] * s[..., 2] - s[..., 1] * s[..., 3]) + s[..., 4] ** 2


def counted_steps(H, freq, gamma):
    """[(t, discount)] of the steps t >= 1 whose reward enters the cost, in order."""
    out, discount = [], 1.0
    for t in range(1, H + 1):
        if t % freq == 0:
            discount *= gamma
            out.append((t, discount))
    return out


def rollout(case: Case, phi, W, s0, eps, H=None, freq=None, gamma=GAMMA, dtype=torch.float64, want_grad=True):
    """dict(cost, grad (D_pol,), states (H + 1, K, S), actions (H, K, A), min_sd) as NumPy arrays of `dtype`."""
    H = case.H if H is None else H
    freq = default_freq(H) if freq is None else freq
    phi_t = torch.tensor(np.asarray(phi), dtype=dtype, requires_grad=want_grad)
    W_t, s, eps_t = (torch.tensor(np.asarray(v), dtype=dtype) for v in (W, s0, eps))
    states, actions = [s], []
    cost = -reward(case.reward, s, 0).mean()
    discount, min_sd = 1.0, np.inf
    for t in range(1, H + 1):
        a = _mlp_shared(phi_t, case.pol_dims, case.pol_acts, s)
        y = _mlp_per_row(W_t, case.dyn_dims, case.dyn_acts, torch.cat([s, a], dim=1))
        m = y.mean(dim=0)
        sd = torch.sqrt(((y - m) ** 2).mean(dim=0))
        min_sd = min(min_sd, float(sd.detach().min()))
        s = m + sd * eps_t[t - 1]
        states.append(s)
        actions.append(a)
        if t % freq == 0:
            discount *= gamma
            cost = cost - discount * reward(case.reward, s, t).mean()
    grad = None
    if want_grad:
        cost.backward()
        grad = phi_t.grad.numpy().copy()
    return dict(cost=float(cost.detach()), grad=grad, states=torch.stack(states).detach().numpy(),
                actions=torch.stack(actions).detach().numpy(), min_sd=min_sd)


_REF = {}


def reference(name: str):
    """The float64 rollout of a case on its seeded inputs, computed once and shared: (inputs, result).  Read-only."""
    if name not in _REF:
        inp = make_inputs(CASE[name])
        res = rollout(CASE[name], **inp)
        for v in list(inp.values()) + [res["grad"], res["states"], res["actions"]]:
            v.setflags(write=False)
        _REF[name] = (inp, res)
    return _REF[name]


def adam_step(phi, m, v, grad, t, lr):
    """One Keras-Adam update (beta_1 0.9, beta_2 0.999, epsilon 1e-7), float64; returns (phi, m, v)."""
    lr_t = lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
    m = m + (grad - m) * (1.0 - 0.9)
    v = v + (grad * grad - v) * (1.0 - 0.999)
    return phi - lr_t * m / (np.sqrt(v) + 1e-7), m, v
