"""Deep-PILCO (the surface of Pyesian/dynamics/deep_pilco.py): a dynamics BNN trained by one of the package's optimizers
on the transitions seen so far, and a policy network improved by differentiating a particle rollout through K draws of
that BNN.  The rollout, its gradient and the policy's Adam step are one chain of HIP kernels (engine.PilcoPlan,
csrc/pyz_pilco.h); everything here is plumbing around it.

Network templates are a compat ``tensorflow.keras.Sequential`` of hidden ``Dense`` layers, or a list of
``(units, activation)`` pairs; the input and the output layer are added from the environment's spaces.  A policy template
may also hold ``RBF(units, gamma)`` layers (the reference's policy: ``Sequential([RBF(80, 0.5)])``)."""

from __future__ import annotations

import json

import numpy as np

from ..datasets import Dataset
from ..nn.model import PolicyNet, model_from_json, sequential_json
from .control import Control, Policy
from .rewards import MIN_STATE, all_rewards

DEFAULT_RANDOM_EPOCHS = 5


class RBF:
    """The radial-basis hidden layer of a policy template (deep_pilco.py:28-51): h[n] = exp(-gamma * sum_k (x[k] -
    mean[k][n])^2) with one trainable variable `mean` (in, units), drawn uniform in [-0.05, 0.05), and no bias.  gamma is a
    constant of the layer.  It holds its two arguments; the network is built by complete_model."""

    def __init__(self, units, gamma, **kwargs):
        self.units, self.gamma = int(units), float(gamma)

    def __repr__(self):
        return f"RBF({self.units}, {self.gamma})"


def template_layers(template):
    """A template's hidden layers: (units, activation name) of a Dense layer, the RBF object of an RBF layer."""
    if template is None:
        return []
    if isinstance(template, (list, tuple)):
        return [l if isinstance(l, RBF) else (int(l[0]), str(l[1])) for l in template]
    layers = getattr(template, "_layers", None)
    if layers is None:
        layers = template.layers
    out = []
    for layer in layers:
        if isinstance(layer, RBF):
            out.append(layer)
            continue
        if not hasattr(layer, "units"):
            raise ValueError("a network template holds Dense and RBF layers only")
        out.append((int(layer.units), str(getattr(layer, "activation", None) or "linear")))
    return out


def complete_model(template, ipd, opd, out_activation):
    """The DenseNet input ipd -> the template's hidden layers -> Dense(opd[0], out_activation); with an RBF layer among
    them, the PolicyNet of the same shape."""
    hidden = template_layers(template)
    if any(isinstance(l, RBF) for l in hidden):
        layers = [("rbf", l.units, l.gamma) if isinstance(l, RBF) else ("dense", l[0], l[1]) for l in hidden]
        return PolicyNet(int(np.prod(ipd)), layers, int(opd[0]), out_activation)
    units = [u for u, _ in hidden] + [int(opd[0])]
    acts = [a for _, a in hidden] + [out_activation]
    return model_from_json(sequential_json(tuple(int(d) for d in ipd), units, acts))


class NNPolicy(Policy):
    """A policy network of Dense and RBF hidden layers; hyperparams may carry ``lr`` (default 1e-3) for its Adam optimizer.
    The parameters, the two Adam moments and the step count live on the device; ``network`` holds a host copy for ``act``."""

    def __init__(self, network, hyperparams):
        super().__init__()
        self.network = network
        self.hyperparams = hyperparams
        self.model_ready = False

    def setup(self, env, ipd):
        params = getattr(self.hyperparams, "_params", {})
        self.learning_rate = float(params.get("lr", 1e-3))
        if not self.model_ready:
            Policy.setup(self, env)
            self.network = complete_model(self.network, ipd, self.action_fd, self.oact)
            self.model_ready = True
            self._phi = self._m = self._v = None
            self.adam_t = 0

    def _device_state(self):
        import torch
        if self._phi is None:
            self._phi = torch.as_tensor(self.network.weights_flat.copy()).cuda()
            self._m, self._v = torch.zeros_like(self._phi), torch.zeros_like(self._phi)
        return self._phi, self._m, self._v

    def _optimize_step(self, plan, check_converge=False, **rollout):
        """One fused rollout + Adam update through `plan` (engine.PilcoPlan.policy_step); returns (cost, grad) on the
        device.  Convergence checking is not implemented (nor is it in the reference): check_converge returns False."""
        phi, m, v = self._device_state()
        self.adam_t += 1
        cost, grad = plan.policy_step(phi, m, v, self.adam_t, lr=self.learning_rate, **rollout)
        self.network.set_flat(phi.cpu().numpy())
        return cost, grad

    def take(self, actions):
        """What the environment is given for each row of network outputs: for a discrete space the index of the first
        largest probability, counted from the space's start; for a box the output clipped to the space's range."""
        actions = np.asarray(actions)
        if self.oact == "softmax":
            return [np.asarray(self.range[0] + int(np.argmax(a))).astype(self.dtype) for a in actions]
        low, high = self.range
        return [np.clip(a, low.reshape(-1), high.reshape(-1)).astype(self.dtype).reshape(self.action_d) for a in actions]

    def act(self, states, take=True):
        """(actions, action_takes): the network's outputs for a batch of states and, with take, what the environment is
        given for each (else an empty list)."""
        actions = self.network(np.asarray(states, dtype=np.float32).reshape(len(states), -1))
        return actions, (self.take(actions) if take else [])


class DynamicsTraining:
    """Learns the transition model f(state, action) -> next state with `optimizer` (SWAG, BBB, HMC, ...).
    data_specs: {"loss": a loss class, "likelihood": "Regression"}; template: the hidden layers; hyperparams: the
    optimizer's.  ``compile_more`` takes the optimizer's extra compile keywords (SWAG's starting_model, ...)."""

    def __init__(self, optimizer, data_specs: dict, template=None, hyperparams=None):
        self.optimizer, self.template = optimizer, template
        self.hyperparams = hyperparams
        self.data_specs = data_specs
        self.features, self.targets = [], []
        self.start = False
        self.model_ready = template is None
        self.rems = {}

    def _create_model(self, ipd, opd):
        if self.model_ready:
            return
        if any(isinstance(l, RBF) for l in template_layers(self.template)):
            raise ValueError("an RBF layer belongs to a policy template: the dynamics model is a Dense network")
        self.model = complete_model(self.template, ipd, opd, out_activation="linear")

    def compile_more(self, extra):
        self.rems = dict(extra)

    def _window(self, features, targets):
        """The data-window rule: once the stored transitions outnumber a trial's fifty to one the store is cut from its
        own length on, i.e. emptied, before the trial is appended."""
        if len(self.features) / len(features) > 50:
            self.targets = self.targets[len(self.features):]
            self.features = self.features[len(self.features):]
        self.features += features
        self.targets += targets

    def _train(self, features, targets, opd, n_epochs):
        """Appends a trial's transitions and retrains: a fresh optimizer of the same class is compiled on everything
        stored (starting from the previous result where the optimizer takes a starting_model) and trained quietly, which
        is the device-resident run."""
        self._window(features, targets)
        x = np.asarray(self.features, dtype=np.float32)
        y = np.asarray(self.targets, dtype=np.float32)
        dataset = Dataset((x, y), self.data_specs["loss"], self.data_specs["likelihood"], target_dim=int(opd[0]),
                          train_proportion=1.0, test_proportion=0.0, valid_proportion=0.0)
        config = self.optimizer._model_config if self.model_ready else self.model.to_json()
        hyperparams = self.hyperparams if self.hyperparams is not None else self.optimizer._hyperparameters
        extra = dict(self.rems)
        if self.start and "starting_model" in extra:
            extra["starting_model"] = self.optimizer.result()._model
        fresh = type(self.optimizer)()
        fresh.compile(hyperparams, config, dataset, verbose=False, **extra)
        fresh.train(n_epochs)
        self.optimizer = fresh
        self.start = True


class BayesianDynamics(Control):
    """The Deep-PILCO loop.  learn_config = (training iterations of the dynamics model per epoch, particles, discount).
    seed: of the rollouts' unit normals (Philox stream STREAM_PILCO, one step per policy update)."""

    def __init__(self, env, horizon: int, dyn_training: DynamicsTraining, policy: NNPolicy, rew_name, learn_config: tuple,
                 seed: int = 0):
        super().__init__(env, horizon, policy)
        if rew_name not in all_rewards:
            raise ValueError(f"unknown reward {rew_name!r}: one of {sorted(all_rewards)}")
        if self.state_fd[0] < MIN_STATE[rew_name]:
            raise ValueError(f"reward {rew_name!r} reads {MIN_STATE[rew_name]} state entries, the environment has {self.state_fd[0]}")
        self.policy.setup(self.env, self.state_fd)
        dyn_training._create_model((self.state_fd[0] + policy.action_fd[0],), (self.state_fd[0],))
        self.dyn_training = dyn_training
        self.rew_name = rew_name
        self.state_reward = all_rewards[rew_name]
        if learn_config:
            self.dyntrain_ep, self.kp, self.gamma = learn_config
        self.seed = int(seed)
        self.updates = 0
        self._plan = self._bufs = self._stream = None

    def _sample_initial(self):
        sample, info = self.env.reset(options=None)
        return sample

    def _t_reward(self, states, t):
        return float(np.mean(self.state_reward(np.asarray(states), t)))

    def _execute(self, use_policy=True):
        """One trial as (features [state, action], targets next state) of the dynamics model."""
        states, actions = super()._execute(use_policy=use_policy)
        flat = [np.asarray(s, dtype=np.float32).reshape(-1) for s in states]
        features = [np.concatenate([s, np.asarray(a, dtype=np.float32).reshape(-1)]) for s, a in zip(flat[:-1], actions)]
        return features, flat[1:]

    def _rollout_inputs(self):
        """K weight draws of the dynamics BNN, K initial states and the rollout's unit normals, in buffers that stay where
        they are from update to update (the captured graph of the rollout holds their addresses)."""
        import torch
        from .. import _lib, engine
        K, S = int(self.kp), self.state_fd[0]
        bnn = self.dyn_training.optimizer.result()
        if self._plan is None:
            net = self.policy.network
            self._plan = engine.PilcoPlan(net if isinstance(net, PolicyNet) else net.spec, bnn._model.spec, K, self.horizon)
            f32 = dict(dtype=torch.float32, device="cuda")
            self._bufs = (torch.empty((K, self._plan.D_dyn), **f32), torch.empty((K, S), **f32),
                          torch.empty((self.horizon, K, S), **f32))
            self._stream = torch.cuda.Stream()          # (graph replay needs a stream of its own)
        W, s0, eps = self._bufs
        W.copy_(bnn.sample_weights_device(K))
        s0.copy_(torch.as_tensor(np.stack([np.asarray(self._sample_initial(), dtype=np.float32).reshape(-1)
                                           for _ in range(K)])))
        engine.fill_normal(eps, self.seed, _lib.STREAM_PILCO, self.updates)
        return W, s0, eps

    def _policy_update(self, ep, record_file, freq, check_converge=False):
        import torch
        W, s0, eps = self._rollout_inputs()
        self._stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._stream):
            cost, grad = self.policy._optimize_step(self._plan, check_converge=check_converge, W=W, s0=s0, eps=eps,
                                                    horizon=self.horizon, gamma=self.gamma, reward=self.rew_name, freq=freq)
            self._stream.synchronize()
        self.updates += 1
        actions = self._plan._actions[:self.horizon, :3].cpu().numpy()
        n_last = self.policy.network.dims[-1]
        with open(record_file, "a") as f:
            f.write("Learning epoch " + str(ep) + "\n; Actions hor: ")
            for t in range(freq, self.horizon + 1, freq):
                f.write(str([str(a) + "," for a in actions[t - 1]]))
            f.write("\nTotal cost: " + str(float(cost.item())) + "\n")
            f.write("Gradient sample: " + str(grad[-n_last:].cpu().numpy()) + ", length " +
                    str(len(self.policy.network.trainable_variables)) + "\n")
        return False

    def learn(self, nb_epochs, record_file, random_ep):
        """nb_epochs epochs of: one trial in the environment (random actions while ep <= random_ep, None: 5), retraining
        of the dynamics model on all transitions, and -- past the random epochs -- one policy update from a rollout of
        `horizon` steps whose every freq-th step's reward is counted, freq = max(int(horizon / 25), 1).  Each policy update
        appends to record_file "Learning epoch <ep>", the actions of three particles at the counted steps,
        "Total cost: <cost>" and "Gradient sample: <the last bias' gradient>, length <number of variables>"."""
        from ..engine import PilcoPlan
        freq = PilcoPlan.default_freq(self.horizon)
        random_ep = DEFAULT_RANDOM_EPOCHS if not random_ep else int(random_ep)

        def step(ep, check_converge=False):
            use_policy = ep > random_ep
            xs, ys = self._execute(use_policy=use_policy)
            self.dyn_training._train(xs, ys, self.state_fd, self.dyntrain_ep)
            if not use_policy:
                return None
            return self._policy_update(ep, record_file, freq, check_converge=check_converge)

        open(record_file, "w").close()
        if nb_epochs:
            for ep in range(1, nb_epochs + 1):
                step(ep)
        else:
            raise ValueError("nb_epochs is required: the policy has no convergence test to stop an open-ended run")

    def store(self, pref, tot_epochs):
        """Writes <pref>agent.json: learn_config, rew_name, horizon, likelihood, tot_epochs and the loss's name."""
        loss = self.dyn_training.data_specs["loss"]
        info = {"learn_config": (self.dyntrain_ep, self.kp, self.gamma), "rew_name": self.rew_name, "horizon": self.horizon,
                "likelihood": self.dyn_training.data_specs["likelihood"], "tot_epochs": tot_epochs,
                "loss": getattr(loss, "__name__", type(loss).__name__)}
        with open(pref + "agent.json", "w") as f:
            json.dump(info, f)
