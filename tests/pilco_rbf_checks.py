"""Float64 restatement of the Deep-PILCO policy update for policies with RBF hidden layers
(Pyesian/dynamics/deep_pilco.py:28-51 for the layer, :247-326 for the update), on torch CPU autograd, and the table of
cases of test_pilco_rbf_host.py / test_gpu_pilco_rbf.py.  The rollout, the dynamics network, the rewards and the Adam step
are pilco_checks'; only the policy differs.  Nothing here touches the library under test.

  RBF(units, gamma):  h[n] = exp(-gamma * sum_k (x[k] - mean[k][n])^2),  mean (in, units), no bias
  flat layout of phi: layers in network order; an RBF layer's means row-major (in, units), a Dense layer's kernel
  (in, out) row-major then its bias.

Draws of phi: means N(0, 0.5^2), Dense kernels N(0, 1 / fan_in), biases N(0, 0.1^2).  Means at Keras' +-0.05 would make
every unit's output ~ 1 for the small states of these cases, and a wrong distance would barely show."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

import pilco_checks as pc

GAMMA = pc.GAMMA


@dataclass(frozen=True)
class Case:
    name: str
    S: int
    A: int
    K: int
    H: int
    pol_hidden: Tuple[tuple, ...]       # ("rbf", units, gamma) | ("dense", units, activation)
    pol_out: str
    dyn_hidden: Tuple[int, ...]
    dyn_hidden_act: str
    reward: str

    @property
    def pol_dims(self):
        return (self.S,) + tuple(l[1] for l in self.pol_hidden) + (self.A,)

    @property
    def pol_kinds(self):
        return tuple(l[0] for l in self.pol_hidden) + ("dense",)

    @property
    def pol_acts(self):
        return tuple("linear" if l[0] == "rbf" else l[2] for l in self.pol_hidden) + (self.pol_out,)

    @property
    def pol_gammas(self):
        return tuple(float(l[2]) if l[0] == "rbf" else 0.0 for l in self.pol_hidden) + (0.0,)

    @property
    def dyn_dims(self):
        return (self.S + self.A,) + self.dyn_hidden + (self.S,)

    @property
    def dyn_acts(self):
        return (self.dyn_hidden_act,) * len(self.dyn_hidden) + ("linear",)

    @property
    def freq(self):
        return pc.default_freq(self.H)


CASES = [
    Case("rbf_min", 4, 1, 2, 1, (("rbf", 3, 0.5),), "linear", (7,), "relu", "Cart"),
    Case("rbf_cart", 4, 2, 5, 8, (("rbf", 8, 0.5),), "softmax", (16,), "relu", "Cart"),
    Case("rbf_odd", 6, 3, 33, 26, (("rbf", 33, 0.5),), "softmax", (65,), "relu", "Acb 2 factors"),
    Case("rbf_wide", 6, 3, 3, 4, (("rbf", 257, 0.25),), "softmax", (16,), "tanh", "Acb 2 factors"),
    Case("rbf_then_dense", 4, 2, 5, 8, (("rbf", 10, 1.5), ("dense", 12, "tanh")), "softmax", (16,), "relu", "Cart"),
    Case("dense_then_rbf", 4, 2, 5, 8, (("dense", 9, "tanh"), ("rbf", 17, 1.5)), "softmax", (16,), "relu", "Cart"),
    Case("rbf_box", 4, 1, 32, 32, (("rbf", 16, 2.0),), "linear", (64, 32), "tanh", "Cart"),
    Case("rbf_example", 6, 3, 32, 32, (("rbf", 80, 0.5),), "softmax", (512, 256), "relu", "Acb 2 factors"),
]
CASE = {c.name: c for c in CASES}
# The seed of every case's inputs.  A rollout through relu dynamics is only piecewise smooth in phi: where a draw leaves a
# pre-activation within float32 rounding of its kink, the float32 restatement's gradient already differs from the float64
# one by far more than rounding (seed 0: 3e-4 of the maximum on `rbf_example`, 5e-6 on `rbf_cart`), and such inputs
# say nothing about a kernel's arithmetic.  With seed 2 the float32 restatement stays within 4e-7 * max |ref| on every
# case, min_sd >= 1e-2 and the RBF-mean slice of every gradient has a maximum >= 9e-3 (test_pilco_rbf_host.py asserts
# the looser figures that every later check relies on).
SEED = 2


def layer_slices(case):
    """The flat slice of phi of every policy layer."""
    out, off = [], 0
    for i, o, kind in zip(case.pol_dims[:-1], case.pol_dims[1:], case.pol_kinds):
        n = i * o if kind == "rbf" else (i + 1) * o
        out.append(slice(off, off + n))
        off += n
    return out


def n_params(case):
    return layer_slices(case)[-1].stop


def draw_phi(rng, case):
    parts = []
    for i, o, kind in zip(case.pol_dims[:-1], case.pol_dims[1:], case.pol_kinds):
        if kind == "rbf":
            parts.append(rng.normal(size=(i, o)).ravel() * 0.5)
        else:
            parts.append(rng.normal(size=(i, o)).ravel() / np.sqrt(i))
            parts.append(rng.normal(size=o) * 0.1)
    return np.concatenate(parts)


def make_inputs(case: Case, seed=SEED):
    """float64 inputs of a case: phi (D_pol,), and W (K, D_dyn), s0 (K, S) uniform in +-0.05, eps (H, K, S) unit normals
    drawn as pilco_checks.make_inputs draws them."""
    rng = np.random.default_rng([seed, 1000 + CASES.index(case)])
    phi = draw_phi(rng, case)
    W = np.stack([pc.draw_flat(rng, case.dyn_dims, 0.7) for _ in range(case.K)])
    s0 = rng.uniform(-0.05, 0.05, size=(case.K, case.S))
    eps = rng.normal(size=(case.H, case.K, case.S))
    return dict(phi=phi, W=W, s0=s0, eps=eps)


def rbf_forward(x, mean, gamma):
    """deep_pilco.py:45-48 on x (rows, in), mean (in, units)."""
    diff = x.unsqueeze(-1) - mean
    norm = (diff ** 2).sum(dim=1)
    return torch.exp(-1 * gamma * norm)


def policy(case, phi, x):
    """x (rows, S) through the policy under the flat phi."""
    for sl, i, o, kind, act, gamma in zip(layer_slices(case), case.pol_dims[:-1], case.pol_dims[1:], case.pol_kinds,
                                          case.pol_acts, case.pol_gammas):
        th = phi[sl]
        if kind == "rbf":
            x = rbf_forward(x, th.reshape(i, o), gamma)
        else:
            x = pc._act(x @ th[:i * o].reshape(i, o) + th[i * o:], act)
    return x


def rollout(case, phi, W, s0, eps, H=None, freq=None, gamma=GAMMA, dtype=torch.float64, want_grad=True):
    """pilco_checks.rollout with this module's policy: dict(cost, grad (D_pol,), states (H + 1, K, S), actions (H, K, A),
    min_sd) as NumPy arrays of `dtype`."""
    H = case.H if H is None else H
    freq = pc.default_freq(H) if freq is None else freq
    phi_t = torch.tensor(np.asarray(phi), dtype=dtype, requires_grad=want_grad)
    W_t, s, eps_t = (torch.tensor(np.asarray(v), dtype=dtype) for v in (W, s0, eps))
    states, actions = [s], []
    cost = -pc.reward(case.reward, s, 0).mean()
    discount, min_sd = 1.0, np.inf
    for t in range(1, H + 1):
        a = policy(case, phi_t, s)
        y = pc._mlp_per_row(W_t, case.dyn_dims, case.dyn_acts, torch.cat([s, a], dim=1))
        m = y.mean(dim=0)
        sd = torch.sqrt(((y - m) ** 2).mean(dim=0))
        min_sd = min(min_sd, float(sd.detach().min()))
        s = m + sd * eps_t[t - 1]
        states.append(s)
        actions.append(a)
        if t % freq == 0:
            discount *= gamma
            cost = cost - discount * pc.reward(case.reward, s, t).mean()
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


adam_step = pc.adam_step
