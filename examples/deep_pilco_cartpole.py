"""Deep-PILCO on the built-in NumPy CartPole: a SWAG dynamics model, a softmax policy, K particles.

    python examples/deep_pilco_cartpole.py [epochs] [--rbf]

Epochs 1..random_ep drive the cart with random actions and only train the dynamics model; every later epoch also improves
the policy by one Adam step on the gradient of a particle rollout (one chain of HIP kernels, engine.PilcoPlan).
--rbf: the policy's hidden layer is RBF(16, 0.5), the radial-basis layer of the reference's own example, instead of
Dense(16, tanh)."""

import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_inference_for_nn_amd.dynamics import RBF, BayesianDynamics, DynamicsTraining, NNPolicy  # noqa: E402
from bayesian_inference_for_nn_amd.dynamics.envs import CartPole  # noqa: E402
from bayesian_inference_for_nn_amd.losses import MeanSquaredError  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers import SWAG  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters  # noqa: E402


def main(epochs=6, horizon=25, particles=16, random_ep=2, rbf=False):
    training = DynamicsTraining(SWAG(), {"loss": MeanSquaredError, "likelihood": "Regression"},
                                template=[(64, "relu"), (32, "relu")],
                                hyperparams=HyperParameters(lr=5e-3, batch_size=16, k=8, scale=1.0, frequency=2))
    policy = NNPolicy([RBF(16, 0.5)] if rbf else [(16, "tanh")], HyperParameters(lr=1e-2))
    agent = BayesianDynamics(CartPole(seed=0), horizon, training, policy, "Cart", (200, particles, 0.95))
    training.compile_more({"starting_model": training.model})
    out = tempfile.mkdtemp(prefix="deep_pilco_")
    record = os.path.join(out, "record.txt")
    agent.learn(epochs, record, random_ep)
    agent.store(out + os.sep, epochs)
    costs = [line.split(":")[1].strip() for line in open(record) if line.startswith("Total cost:")]
    print("policy updates:", len(costs), "costs:", ", ".join(costs))
    print("last trial's actions:", agent.last_takes)
    print("record and agent.json in", out)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--rbf"]
    main(int(args[0]) if args else 6, rbf="--rbf" in sys.argv[1:])
