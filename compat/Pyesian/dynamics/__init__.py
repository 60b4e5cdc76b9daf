"""`Control`, `Policy`, `NNPolicy`, `DynamicsTraining`, `BayesianDynamics`, `RBF` and `all_rewards` are the library's own."""

from bayesian_inference_for_nn_amd.dynamics import (RBF, BayesianDynamics, Control, DynamicsTraining, NNPolicy, Policy,  # noqa: F401
                                                    all_rewards)
