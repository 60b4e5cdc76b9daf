"""CPU checks behind test_gpu_pilco.py: the float64 restatement of the Deep-PILCO policy update (pilco_checks.py) is
itself checked -- its gradient against central finite differences, its inputs against the conditions that keep a case
away from the sqrt singularity, its float32 evaluation against the float64 one -- and the host plumbing of the dynamics
package that needs no GPU."""

import json
import re

import numpy as np
import pytest
import torch

import pilco_checks as pc

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.dynamics import BayesianDynamics, DynamicsTraining, NNPolicy, all_rewards
from bayesian_inference_for_nn_amd.dynamics import control, envs
from bayesian_inference_for_nn_amd.dynamics.deep_pilco import complete_model, template_layers
from bayesian_inference_for_nn_amd.losses import MeanSquaredError
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

NAMES = [c.name for c in pc.CASES]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["min", "cart_softmax"])
def test_restatement_gradient_agrees_with_central_differences(name):
    case = pc.CASE[name]
    inp, ref = pc.reference(name)
    h = 1e-6
    fd = np.zeros_like(inp["phi"])
    for e in range(len(fd)):
        hi, lo = inp["phi"].copy(), inp["phi"].copy()
        hi[e] += h
        lo[e] -= h
        fd[e] = (pc.rollout(case, hi, inp["W"], inp["s0"], inp["eps"], want_grad=False)["cost"] -
                 pc.rollout(case, lo, inp["W"], inp["s0"], inp["eps"], want_grad=False)["cost"]) / (2 * h)
    # central differences in float64 with h = 1e-6: truncation ~ h^2, rounding ~ 1e-16 / h = 1e-10 per unit of cost
    assert np.abs(fd - ref["grad"]).max() <= 1e-7 * max(1.0, np.abs(ref["grad"]).max())


@pytest.mark.parametrize("name", NAMES)
def test_case_inputs_stay_clear_of_the_singularity_and_do_not_diverge(name):
    _, ref = pc.reference(name)
    assert ref["min_sd"] >= 1e-2
    assert np.abs(ref["states"]).max() <= 4.0
    assert np.abs(ref["grad"]).max() > 0.0, "an identically zero gradient checks nothing"
    assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["cost"])


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_is_within_1e_5(name):
    case = pc.CASE[name]
    inp, ref = pc.reference(name)
    r32 = pc.rollout(case, **inp, dtype=torch.float32)
    for key in ("grad", "states", "actions"):
        assert np.abs(r32[key] - ref[key]).max() <= 1e-5 * np.abs(ref[key]).max(), key
    assert abs(r32["cost"] - ref["cost"]) <= 1e-5 * abs(ref["cost"])


def test_case_table_is_the_issues():
    assert NAMES == ["min", "cart_softmax", "acb_two_hidden", "freq2", "odd", "box_linear", "sigmoid", "example"]
    ex = pc.CASE["example"]
    assert (ex.pol_dims, ex.dyn_dims, ex.K, ex.H, ex.freq) == ((6, 80, 3), (9, 512, 256, 6), 32, 32, 1)
    assert pc.CASE["freq2"].freq == 2 and pc.CASE["min"].pol_dims == (4, 1) and pc.CASE["min"].K == 2
    assert all(c.dyn_acts[-1] == "linear" and c.S >= pc.REWARD_MIN_S[c.reward] for c in pc.CASES)


def test_rewards_equal_hand_computed_values():
    s = np.array([0.5, -0.25, 0.125, 2.0, -1.5, 9.0])
    # Cart: -s2 - s3 s2 + t (-s2^2 + 0.2095^2) at t = 3: -0.125 - 0.25 + 3 (-0.015625 + 0.04389025)
    cart = -0.125 - 0.25 + 3 * (-0.015625 + 0.04389025)
    # Acb: 4 - 3 s0 - (s0 s2 - s1 s3) + s4^2 = 4 - 1.5 - (0.0625 + 0.5) + 2.25
    acb = 4 - 1.5 - (0.0625 + 0.5) + 2.25
    for fn in (lambda n, t: float(pc.reward(n, s, t)), lambda n, t: float(all_rewards[n](s, t)),
               lambda n, t: float(pc.reward(n, torch.tensor(s), t))):
        assert fn("Cart", 3) == pytest.approx(cart, rel=1e-14)
        assert fn("Acb 2 factors", 7) == pytest.approx(acb, rel=1e-14)
    assert sorted(all_rewards) == sorted(_lib.REWARD) == ["Acb 2 factors", "Cart"]
    batch = np.stack([s, 2 * s])
    np.testing.assert_allclose(all_rewards["Cart"](batch, 3), [all_rewards["Cart"](s, 3), all_rewards["Cart"](2 * s, 3)])


def test_schedule_counts_the_even_steps_of_h_50_and_starts_at_gamma():
    assert pc.default_freq(50) == 2 and pc.default_freq(24) == 1 and pc.default_freq(1000) == 40 and pc.default_freq(1) == 1
    steps = pc.counted_steps(50, 2, 0.95)
    assert [t for t, _ in steps] == list(range(2, 51, 2))
    assert steps[0] == (2, 0.95) and steps[-1][1] == pytest.approx(0.95 ** 25, rel=1e-12)
    # the restatement uses exactly this schedule: a cost assembled from its states by hand
    case = pc.CASE["freq2"]
    _, ref = pc.reference("freq2")
    cost = -pc.reward(case.reward, ref["states"][0], 0).mean()
    for t, d in steps:
        cost -= d * pc.reward(case.reward, ref["states"][t], t).mean()
    assert cost == pytest.approx(ref["cost"], rel=1e-12)


def test_adam_step_is_keras_adam():
    g = np.array([0.5, -2.0])
    phi, m, v = pc.adam_step(np.array([1.0, 1.0]), np.zeros(2), np.zeros(2), g, 1, 0.1)
    np.testing.assert_allclose(m, 0.1 * g, rtol=1e-12)
    np.testing.assert_allclose(v, 0.001 * g * g, rtol=1e-12)
    # at t = 1 the bias corrections cancel the moments' factors: the step is lr * sign(g) up to epsilon
    np.testing.assert_allclose(phi, 1.0 - 0.1 * np.sign(g), rtol=1e-5)


# ------------------------------------------------------------------ host plumbing
def test_space_flattening():
    assert control._space_flat(()) == (1,)
    assert control._space_flat((4,)) == (4,)
    assert control._space_flat((2, 3, 5)) == (30,)
    assert control.is_discrete(envs.Discrete(3)) and not control.is_discrete(envs.Box(-1.0, 1.0, shape=(2,)))


class _Env:
    def __init__(self, action_space, obs=4):
        self.action_space = action_space
        self.observation_space = envs.Box(-1.0, 1.0, shape=(obs,))


def test_discrete_action_takes_are_the_first_arg_max_from_the_spaces_start():
    pol = NNPolicy([(8, "tanh")], HyperParameters(lr=0.01))
    pol.setup(_Env(envs.Discrete(3, start=2)), (4,))
    assert (pol.oact, pol.action_fd, pol.range, pol.learning_rate) == ("softmax", (3,), (2, 4), 0.01)
    assert pol.network.dims == (4, 8, 3) and pol.network.acts == ("tanh", "softmax")
    takes = pol.take(np.array([[0.2, 0.5, 0.3], [0.4, 0.4, 0.2], [0.1, 0.1, 0.8]]))
    assert [int(t) for t in takes] == [3, 2, 4] and all(t.dtype == np.int64 for t in takes)


def test_box_action_takes_are_clipped_to_the_range():
    pol = NNPolicy(None, HyperParameters())
    pol.setup(_Env(envs.Box(np.array([-1.0, 0.0]), np.array([1.0, 2.0]))), (4,))
    assert (pol.oact, pol.action_fd, pol.learning_rate) == ("linear", (2,), 1e-3) and pol.network.dims == (4, 2)
    takes = pol.take(np.array([[-3.0, 3.0], [0.5, -0.5]]))
    np.testing.assert_array_equal(takes, [[-1.0, 2.0], [0.5, 0.0]])
    assert takes[0].dtype == np.float32 and takes[0].shape == (2,)
    pos = NNPolicy(None, HyperParameters())
    pos.setup(_Env(envs.Box(0.0, 1.0, shape=(1,))), (4,))
    assert pos.oact == "relu"


def test_templates_from_pairs_and_from_a_compat_sequential():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat", "tensorflow", "__init__.py")
    mod_spec = importlib.util.spec_from_file_location("pyz_compat_tensorflow", path)
    tf = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(tf)
    seq = tf.keras.Sequential()
    seq.add(tf.keras.layers.Dense(16, "relu"))
    seq.add(tf.keras.layers.Dense(8, activation=tf.keras.activations.tanh))
    assert template_layers(seq) == template_layers([(16, "relu"), (8, "tanh")]) == [(16, "relu"), (8, "tanh")]
    net = complete_model(seq, (6,), (4,), "linear")
    assert net.dims == (6, 16, 8, 4) and net.acts == ("relu", "tanh", "linear")


class _StubOptimizer:
    """Records what DynamicsTraining hands to a fresh optimizer of its class."""
    log = []

    def compile(self, hyperparameters, model_config, dataset, verbose=True, **kwargs):
        self.n = dataset.train_size
        _StubOptimizer.log.append(("compile", self.n, verbose, sorted(kwargs)))

    def train(self, n):
        _StubOptimizer.log.append(("train", n))

    def result(self):
        return type("R", (), {"_model": ("model after", self.n)})()


def test_data_window_rule_with_a_stub_optimizer():
    _StubOptimizer.log = []
    dt = DynamicsTraining(_StubOptimizer(), {"loss": MeanSquaredError, "likelihood": "Regression"}, template=[(4, "relu")],
                          hyperparams=HyperParameters(lr=0.1))
    dt.compile_more({"starting_model": "first"})
    dt._create_model((5,), (4,))
    assert dt.model.dims == (5, 4, 4) and dt.model.acts == ("relu", "linear")
    trial = lambda n: ([np.zeros(5, dtype=np.float32)] * n, [np.zeros(4, dtype=np.float32)] * n)  # noqa: E731
    dt._train(*trial(100), (4,), 7)
    assert len(dt.features) == len(dt.targets) == 100
    dt._train(*trial(1), (4,), 7)                       # 100 / 1 > 50: the store is emptied, then the trial appended
    assert len(dt.features) == len(dt.targets) == 1
    dt._train(*trial(2), (4,), 7)                       # 1 / 2: kept
    assert len(dt.features) == 3
    dt.features, dt.targets = dt.features * 34, dt.targets * 34          # 102 stored
    dt._train(*trial(2), (4,), 7)                       # 102 / 2 = 51 > 50
    assert len(dt.features) == 2
    dt.features, dt.targets = dt.features * 50, dt.targets * 50          # 100 stored
    dt._train(*trial(2), (4,), 7)                       # exactly 50: kept
    assert len(dt.features) == 102
    compiles = [e for e in _StubOptimizer.log if e[0] == "compile"]
    assert [e[1] for e in compiles] == [100, 1, 3, 2, 102]           # a fresh optimizer sees everything stored
    assert all(e[2] is False and e[3] == ["starting_model"] for e in compiles)
    assert _StubOptimizer.log.count(("train", 7)) == 5 and isinstance(dt.optimizer, _StubOptimizer)


def test_cartpole_is_deterministic_under_a_seed():
    def run(seed):
        env = envs.CartPole(seed=seed)
        obs = [env.reset()[0]]
        for k in range(40):
            o, r, term, trunc, info = env.step(k % 2 if k < 20 else 1)
            obs.append(o)
        obs.append(env.reset()[0])
        return np.stack(obs), term
    a, term = run(3)
    b, _ = run(3)
    c, _ = run(4)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c)
    assert a.dtype == np.float32 and a.shape == (42, 4) and np.abs(a[0]).max() <= 0.05 and np.abs(a[-1]).max() <= 0.05
    assert term, "twenty pushes to the right must tip the pole past 12 degrees"
    env = envs.CartPole(seed=0)
    assert env.observation_space.shape == (4,) and env.action_space.n == 2 and env.action_space.shape == ()
    s0, _ = env.reset()
    s1 = env.step(1)[0]
    # one Euler step by hand: positions move by tau * velocity
    np.testing.assert_allclose(s1[[0, 2]], s0[[0, 2]] + 0.02 * s0[[1, 3]], rtol=1e-6)
    assert s1[1] > s0[1] and s1[3] < s0[3]             # a push to the right accelerates the cart and tips the pole left
    with pytest.raises(ValueError):
        env.step(2)


def test_agent_json_names_the_loss_and_writes_no_pickle(tmp_path):
    dt = DynamicsTraining(_StubOptimizer(), {"loss": MeanSquaredError, "likelihood": "Regression"}, template=[(4, "relu")])
    bd = BayesianDynamics(envs.CartPole(seed=0), 10, dt, NNPolicy([(8, "tanh")], HyperParameters(lr=0.01)), "Cart",
                          (20, 8, 0.95))
    assert dt.model.dims == (6, 4, 4) and bd.policy.network.dims == (4, 8, 2)
    bd.store(str(tmp_path) + "/", 3)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["agent.json"]
    info = json.loads((tmp_path / "agent.json").read_text())
    assert info == {"learn_config": [20, 8, 0.95], "rew_name": "Cart", "horizon": 10, "likelihood": "Regression",
                    "tot_epochs": 3, "loss": "MeanSquaredError"}
    with pytest.raises(ValueError):
        BayesianDynamics(envs.CartPole(seed=0), 10, dt, NNPolicy(None, HyperParameters()), "Acb 2 factors", (20, 8, 0.95))
    with pytest.raises(ValueError):
        BayesianDynamics(envs.CartPole(seed=0), 10, dt, NNPolicy(None, HyperParameters()), "Nope", (20, 8, 0.95))


def test_random_trial_gives_features_and_targets_of_the_dynamics_model():
    dt = DynamicsTraining(_StubOptimizer(), {"loss": MeanSquaredError, "likelihood": "Regression"}, template=[(4, "relu")])
    bd = BayesianDynamics(envs.CartPole(seed=1), 6, dt, NNPolicy(None, HyperParameters()), "Cart", (20, 8, 0.95))
    xs, ys = bd._execute(use_policy=False)
    assert len(xs) == len(ys) == 6 and all(x.shape == (6,) for x in xs) and all(y.shape == (4,) for y in ys)
    for k in range(5):
        np.testing.assert_array_equal(xs[k + 1][:4], ys[k])         # a target is the next feature's state
        assert xs[k][4:].min() >= 0.0 and xs[k][4:].sum() <= 1.0      # the gaps of two sorted uniforms
    assert all(t in (0, 1) for t in bd.last_takes)


def test_stream_id_is_declared_in_the_rng_header():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = open(os.path.join(root, "bayesian_inference_for_nn_amd", "csrc", "pyz_rng.h")).read()
    assert re.search(r"#define PYZ_STREAM_PILCO 8u", rng) and _lib.STREAM_PILCO == 8
    hdr = open(os.path.join(root, "include", "pyz.h")).read()
    assert "#define PYZ_REWARD_CART 0" in hdr and "#define PYZ_REWARD_ACB 1" in hdr
    assert _lib.REWARD == {"Cart": 0, "Acb 2 factors": 1}
