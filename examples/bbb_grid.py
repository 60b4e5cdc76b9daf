"""The hyper-parameter grid of the reference's BBB_mnist.py -- lr x alpha x batch_size, per hidden width -- on the synthetic
MNIST stand-in, through GridOptimizer: every (lr, alpha) point of a batch size trains as one lane of ONE particle-batched
Bayes-by-Backprop run (BBB.compile's lanes) instead of one compile + train per point.
    python examples/bbb_grid.py [steps]
The hidden width changes the model, so it stays an outer loop; batch sizes make groups of their own inside the objective."""
import sys

from bayesian_inference_for_nn_amd import synth
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.distributions import GaussianPrior
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
from bayesian_inference_for_nn_amd.nn import sequential_json
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import BBBGridObjective, GridOptimizer, HyperParameters, Integer, Real

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
lr_values = [1e-4, 1e-3, 1e-2]
alpha_values = [0.0, 1e-4]
batch_size_values = [500, 1000]
hidden_dims_values = [128, 256]

x, y = synth.mnist_like(12_000)
dataset = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=0)
best = None
for hidden in hidden_dims_values:
    objective = BBBGridObjective(HyperParameters(lr=lr_values[0], alpha=alpha_values[0], batch_size=batch_size_values[0]),
                                 sequential_json(784, [hidden, 10], ["relu", "softmax"]), dataset, steps,
                                 prior=GaussianPrior(0.0, -5.0), metric="val_error", weights="predictive", nb_samples=100, seed=1)
    grid = GridOptimizer()
    grid.compile(objective, Real(0, 1, "lr"), Real(0, 1, "alpha"), Integer(1, 10_000, "batch_size"), n=2, verbose=False,
                 specify={"lr": lr_values, "alpha": alpha_values, "batch_size": batch_size_values})
    grid.optimize()
    point, error = grid.best()
    print(f"hidden {hidden}: {len(grid.results)} points in {len(objective.trainings)} trainings of {objective.trainings} lanes; "
          f"best lr={point[0]}, alpha={point[1]}, batch_size={point[2]}: validation error {error:.4f}")
    if best is None or error < best[0]:
        best = (error, hidden) + point
print(f"best: hidden={best[1]}, lr={best[2]}, alpha={best[3]}, batch_size={best[4]} (validation error {best[0]:.4f})")
