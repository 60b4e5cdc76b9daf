"""``Policy`` and ``Control``: the base classes of Pyesian/dynamics/control.py:14-144.  Environments are duck-typed
(``reset(options=)``, ``step``, ``action_space``, ``observation_space``): gymnasium's classes are recognised with
``isinstance`` when gymnasium can be imported, otherwise a space with ``.n`` is discrete and anything else a box."""

from __future__ import annotations

import random
from abc import ABC, abstractmethod

import numpy as np

try:
    import gymnasium as gym
except ImportError:                 # not a dependency: the spaces of dynamics.envs (or anything shaped like them) do
    gym = None


def _space_flat(shape):
    """The shape of a space flattened to one axis; a scalar space, shape (), has one entry."""
    return (int(np.prod(shape, dtype=np.int64)),)


def is_discrete(space) -> bool:
    if gym is not None and isinstance(space, gym.spaces.Space):
        return isinstance(space, gym.spaces.Discrete)
    return hasattr(space, "n")


class Policy(ABC):
    """Base class of a policy: ``setup`` reads the action space (control.py:21-46)."""

    def __init__(self):
        self.dtype, self.range = None, None

    def setup(self, env):
        aspace = env.action_space
        self.action_d = aspace.shape
        self.action_fd = _space_flat(aspace.shape)
        if is_discrete(aspace):
            start = int(getattr(aspace, "start", 0))
            self.action_fd = (int(aspace.n),)
            self.oact = "softmax"
            self.range = (start, start + int(aspace.n) - 1)
        else:
            low = min(np.asarray(aspace.low).reshape(-1))
            self.oact = "relu" if low >= 0 else "linear"
            self.range = (np.asarray(aspace.low), np.asarray(aspace.high))
        self.dtype = aspace.dtype

    @abstractmethod
    def _optimize_step(self, **kwargs):
        pass

    @abstractmethod
    def act(self, states):
        pass


class Control(ABC):
    """Reinforcement-learning controller over an environment, a horizon and a policy (control.py:61-135)."""

    def __init__(self, env, horizon: int, policy: Policy):
        self.env = env
        self.state_d = env.observation_space.shape
        self.state_fd = _space_flat(self.state_d)
        self.horizon = horizon
        self.policy = policy

    @abstractmethod
    def _sample_initial(self):
        pass

    @abstractmethod
    def _t_reward(self, **kwargs):
        pass

    def _random_action(self):
        """(action as the dynamics net sees it, action as the environment takes it) of the random policy: for a discrete
        space the gaps of n sorted uniforms and their arg-max, for a box a sample of the space (control.py:98-114)."""
        aspace = self.env.action_space
        if is_discrete(aspace):
            probs = sorted(random.random() for _ in range(aspace.n))
            action = np.array([probs[0]] + [probs[i] - probs[i - 1] for i in range(1, aspace.n)], dtype=np.float32)
            return action, int(np.argmax(action))
        action = np.asarray(aspace.sample())
        return action.astype(self.env.observation_space.dtype).reshape(-1), action

    def _execute(self, use_policy=True):
        """One trial of `horizon` steps in the environment: (horizon + 1 states, horizon actions)."""
        state = self._sample_initial()
        all_states, all_actions, takes = [np.asarray(state)], [], []
        for t in range(self.horizon):
            if use_policy:
                actions, action_takes = self.policy.act(np.reshape(state, (1, -1)))
                action, action_take = np.asarray(actions[0]), action_takes[0]
            else:
                action, action_take = self._random_action()
            state, reward, terminated, truncated, info = self.env.step(action_take)
            all_states.append(np.asarray(state))
            all_actions.append(action)
            takes.append(action_take)
        self.last_takes = takes
        return all_states, all_actions

    @abstractmethod
    def learn(self, nb_epochs, **kwargs):
        pass
