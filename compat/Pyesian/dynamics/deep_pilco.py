"""The reference's module path: `from Pyesian.dynamics.deep_pilco import BayesianDynamics, NNPolicy, DynamicsTraining, RBF`."""

from bayesian_inference_for_nn_amd.dynamics.deep_pilco import (RBF, BayesianDynamics, DynamicsTraining, NNPolicy,  # noqa: F401
                                                               complete_model)
