"""A NumPy environment with the gymnasium interface the dynamics package drives (``reset(options=)``, ``step``,
``action_space``, ``observation_space``), so that examples and tests run where gymnasium is not installed."""

from __future__ import annotations

import numpy as np


class Discrete:
    """The part of gymnasium.spaces.Discrete the package reads: n, start, shape (), dtype, sample()."""

    def __init__(self, n: int, start: int = 0, seed=None):
        self.n, self.start, self.shape, self.dtype = int(n), int(start), (), np.dtype(np.int64)
        self._rng = np.random.default_rng(seed)

    def sample(self):
        return int(self.start + self._rng.integers(self.n))


class Box:
    """The part of gymnasium.spaces.Box the package reads: low, high (arrays), shape, dtype, sample()."""

    def __init__(self, low, high, shape=None, dtype=np.float32, seed=None):
        shape = tuple(shape) if shape is not None else np.shape(low)
        self.low = np.broadcast_to(np.asarray(low, dtype=dtype), shape).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype=dtype), shape).copy()
        self.shape, self.dtype = shape, np.dtype(dtype)
        self._rng = np.random.default_rng(seed)

    def sample(self):
        lo, hi = np.maximum(self.low, -1e6), np.minimum(self.high, 1e6)
        return self._rng.uniform(lo, hi).astype(self.dtype)


class CartPole:
    """CartPole-v1's dynamics (Barto, Sutton & Anderson 1983, Euler steps of 0.02 s): observation (x, x', theta, theta'),
    actions 0 (push left) / 1 (push right) with a force of 10 N.  ``reset`` draws every entry uniformly in +-0.05 from the
    generator seeded at construction (or by ``reset(seed=)``).  An episode is never cut short: ``terminated`` reports the
    pole past 12 degrees or the cart past +-2.4, and stepping goes on, as the fixed-horizon trials of Control need."""

    gravity, masscart, masspole, length, force_mag, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
    theta_threshold, x_threshold = 12 * 2 * np.pi / 360, 2.4

    def __init__(self, seed=0):
        high = np.array([2 * self.x_threshold, np.finfo(np.float32).max, 2 * self.theta_threshold, np.finfo(np.float32).max],
                        dtype=np.float32)
        self.observation_space = Box(-high, high, dtype=np.float32, seed=seed)
        self.action_space = Discrete(2, seed=seed)
        self._rng = np.random.default_rng(seed)
        self.state = None

    def reset(self, seed=None, options=None):
        if seed is not None:
            self._rng = np.random.default_rng(seed)
        low, high = (options or {}).get("low", -0.05), (options or {}).get("high", 0.05)
        self.state = self._rng.uniform(low, high, size=4)
        return self.state.astype(np.float32), {}

    def step(self, action):
        action = int(np.asarray(action).reshape(-1)[0])
        if action not in (0, 1):
            raise ValueError(f"action {action!r} is not in Discrete(2)")
        x, x_dot, theta, theta_dot = self.state
        force = self.force_mag if action == 1 else -self.force_mag
        cos, sin = np.cos(theta), np.sin(theta)
        total_mass, polemass_length = self.masspole + self.masscart, self.masspole * self.length
        temp = (force + polemass_length * theta_dot ** 2 * sin) / total_mass
        theta_acc = (self.gravity * sin - cos * temp) / (self.length * (4.0 / 3.0 - self.masspole * cos ** 2 / total_mass))
        x_acc = temp - polemass_length * theta_acc * cos / total_mass
        self.state = np.array([x + self.tau * x_dot, x_dot + self.tau * x_acc, theta + self.tau * theta_dot,
                               theta_dot + self.tau * theta_acc])
        terminated = bool(abs(self.state[0]) > self.x_threshold or abs(self.state[2]) > self.theta_threshold)
        return self.state.astype(np.float32), 1.0, terminated, False, {}
