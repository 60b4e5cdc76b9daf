from bayesian_inference_for_nn_amd.optimizers.hyperparameters import (  # noqa: F401
    BBBGridObjective, Constant, GridOptimizer, HyperParameters, HyperparameterOptimizer, Integer, Number, Parameter, Real, SGLDGridObjective)
