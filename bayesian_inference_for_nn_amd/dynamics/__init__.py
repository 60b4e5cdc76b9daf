"""Model-based reinforcement learning on the package's Bayesian networks: Deep-PILCO (see deep_pilco.py)."""

from .control import Control, Policy  # noqa: F401
from .deep_pilco import RBF, BayesianDynamics, DynamicsTraining, NNPolicy  # noqa: F401
from .rewards import all_rewards  # noqa: F401
