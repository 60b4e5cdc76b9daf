"""CPU checks behind test_gpu_pilco_rbf.py: the float64 restatement of the policy update with RBF layers
(pilco_rbf_checks.py) is itself checked -- its RBF forward against a literal NumPy transcription of the reference's
call(), its gradient against central finite differences, every case for a live gradient in every layer and for the
float32 premise of the GPU bound -- and the host side of the feature: the RBF class, the policy network object, the
rejections and the argument checks of pyz_pilco_create_layers, none of which needs a GPU."""

import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import pilco_checks as pc
import pilco_rbf_checks as rc

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.dynamics import RBF, DynamicsTraining, NNPolicy, envs
from bayesian_inference_for_nn_amd.dynamics.deep_pilco import complete_model, template_layers
from bayesian_inference_for_nn_amd.losses import MeanSquaredError
from bayesian_inference_for_nn_amd.nn.BayesianModel import BayesianModel
from bayesian_inference_for_nn_amd.nn.model import DenseNet, PolicyNet
from bayesian_inference_for_nn_amd.optimizers import SGD
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in rc.CASES]


# ------------------------------------------------------------------ the restatement
def test_rbf_forward_is_the_references_call_transcribed():
    rng = np.random.default_rng(3)
    x, mean, gamma = rng.normal(size=(5, 6)), rng.normal(size=(6, 11)) * 0.5, 0.7
    diff = np.expand_dims(x, -1) - mean                    # bk.expand_dims(inputs) - self.mean
    norm = np.sum(np.power(diff, 2), axis=1)               # bk.sum(bk.pow(diff, 2), axis=1)
    want = np.exp(-1 * gamma * norm)                       # bk.exp(-1 * self.gamma * norm)
    got = rc.rbf_forward(torch.tensor(x), torch.tensor(mean), gamma).numpy()
    assert got.shape == (5, 11)
    np.testing.assert_allclose(got, want, rtol=1e-14)
    # and entry by entry, from the definition
    assert got[2, 4] == pytest.approx(np.exp(-gamma * sum((x[2, k] - mean[k, 4]) ** 2 for k in range(6))), rel=1e-13)


@pytest.mark.parametrize("name", ["rbf_min", "rbf_cart"])
def test_restatement_gradient_agrees_with_central_differences(name):
    case = rc.CASE[name]
    inp, ref = rc.reference(name)
    h = 1e-6
    fd = np.zeros_like(inp["phi"])
    for e in range(len(fd)):
        hi, lo = inp["phi"].copy(), inp["phi"].copy()
        hi[e] += h
        lo[e] -= h
        fd[e] = (rc.rollout(case, hi, inp["W"], inp["s0"], inp["eps"], want_grad=False)["cost"] -
                 rc.rollout(case, lo, inp["W"], inp["s0"], inp["eps"], want_grad=False)["cost"]) / (2 * h)
    # central differences in float64 with h = 1e-6: truncation ~ h^2, rounding ~ 1e-16 / h = 1e-10 per unit of cost
    assert np.abs(fd - ref["grad"]).max() <= 1e-7 * max(1.0, np.abs(ref["grad"]).max())


@pytest.mark.parametrize("name", NAMES)
def test_every_case_is_sound_and_float32_is_within_1e_5(name):
    case = rc.CASE[name]
    inp, ref = rc.reference(name)
    assert ref["min_sd"] >= 4e-3 and np.isfinite(ref["grad"]).all() and np.isfinite(ref["cost"])
    assert np.abs(ref["states"]).max() <= 4.0
    assert len(inp["phi"]) == rc.n_params(case) == len(ref["grad"])
    for sl, kind in zip(rc.layer_slices(case), case.pol_kinds):
        assert np.abs(ref["grad"][sl]).max() > 0.0, f"the {kind} layer at {sl} has an identically zero gradient"
        if kind == "rbf":
            assert np.abs(ref["grad"][sl]).max() >= 3e-3, "a mean gradient this small would hide a wrong distance"
    # the premise of the GPU bound (1e-4 * max |ref|): float32 arithmetic alone stays ten times below it
    r32 = rc.rollout(case, **inp, dtype=torch.float32)
    for key in ("grad", "states", "actions"):
        assert np.abs(r32[key] - ref[key]).max() <= 1e-5 * np.abs(ref[key]).max(), key
    for sl in rc.layer_slices(case):
        assert np.abs(r32["grad"][sl] - ref["grad"][sl]).max() <= 1e-5 * np.abs(ref["grad"][sl]).max(), sl
    assert abs(r32["cost"] - ref["cost"]) <= 1e-5 * abs(ref["cost"])


def test_case_table_is_the_issues():
    assert NAMES == ["rbf_min", "rbf_cart", "rbf_odd", "rbf_wide", "rbf_then_dense", "dense_then_rbf", "rbf_box", "rbf_example"]
    ex = rc.CASE["rbf_example"]
    assert (ex.pol_dims, ex.pol_kinds, ex.pol_gammas, ex.dyn_dims, ex.K, ex.H) == \
        ((6, 80, 3), ("rbf", "dense"), (0.5, 0.0), (9, 512, 256, 6), 32, 32)
    assert rc.n_params(ex) == 6 * 80 + 81 * 3
    assert rc.CASE["rbf_wide"].pol_dims == (6, 257, 3) and rc.CASE["rbf_wide"].pol_gammas[0] == 0.25
    assert rc.CASE["rbf_then_dense"].pol_kinds == ("rbf", "dense", "dense")
    assert rc.CASE["dense_then_rbf"].pol_kinds == ("dense", "rbf", "dense")
    assert rc.CASE["dense_then_rbf"].pol_acts == ("tanh", "linear", "softmax")
    assert all(c.pol_kinds[-1] == "dense" and c.S >= pc.REWARD_MIN_S[c.reward] for c in rc.CASES)


# ------------------------------------------------------------------ the Python surface
def _compat(name):
    path = os.path.join(ROOT, "compat", *name.split("."), "__init__.py")
    if not os.path.exists(path):
        path = os.path.join(ROOT, "compat", *name.split(".")) + ".py"
    spec = importlib.util.spec_from_file_location("pyz_compat_" + name.replace(".", "_"), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rbf_imports_from_both_packages_and_templates_keep_it():
    assert _compat("Pyesian.dynamics").RBF is RBF and _compat("Pyesian.dynamics.deep_pilco").RBF is RBF
    # the reference's import line, with compat/ on the path
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        from Pyesian.dynamics.deep_pilco import BayesianDynamics, DynamicsTraining as DT, NNPolicy as NP, RBF as R  # noqa: F401
        assert R is RBF and NP is NNPolicy and DT is DynamicsTraining
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    layer = RBF(80, 0.5)
    assert (layer.units, layer.gamma) == (80, 0.5)
    assert template_layers([layer]) == [layer] and template_layers([(9, "tanh"), layer]) == [(9, "tanh"), layer]
    tf = _compat("tensorflow")
    seq = tf.keras.Sequential([layer])
    assert template_layers(seq) == [layer]
    seq.add(tf.keras.layers.Dense(12, "tanh"))
    assert template_layers(seq) == [layer, (12, "tanh")]
    with pytest.raises(ValueError, match="no Keras config"):
        seq.to_json()
    # Dense-only templates give what they gave before
    assert type(complete_model([(8, "tanh")], (4,), (2,), "softmax")) is DenseNet


@pytest.mark.parametrize("units", [8, 80])
def test_nnpolicy_setup_builds_the_policy_network(units):
    tf = _compat("tensorflow")
    pol = NNPolicy(tf.keras.Sequential([RBF(units, 0.5)]), HyperParameters(lr=1, batch_size=10))
    pol.setup(envs.CartPole(seed=0), (4,))
    net = pol.network
    assert isinstance(net, PolicyNet) and pol.learning_rate == 1.0
    assert (net.dims, net.acts, net.kinds, net.gammas) == ((4, units, 2), ("linear", "softmax"), ("rbf", "dense"), (0.5, 0.0))
    assert net.n_params == 4 * units + (units + 1) * 2 == len(net.weights_flat) and net.weights_flat.dtype == np.float32
    mean, kernel, bias = net.trainable_variables
    assert mean.shape == (4, units) and kernel.shape == (units, 2) and bias.shape == (2,)
    assert -0.05 <= mean.min() and mean.max() < 0.05 and np.ptp(mean) > 0.05       # Keras 'uniform'
    lim = np.sqrt(6.0 / (units + 2))
    assert np.abs(kernel).max() <= lim and np.abs(kernel).max() > 0.3 * lim and not bias.any()
    # views of the flat vector, in network order
    assert np.array_equal(net.weights_flat[:4 * units].reshape(4, units), mean)
    w = net.get_weights()
    assert len(w) == 3 and w[0] is not mean
    new = [np.full_like(w[0], 0.25), np.full_like(w[1], -2.0), np.array([3.0, 4.0], dtype=np.float32)]
    net.set_weights(new)
    for got, want in zip(net.get_weights(), new):
        assert np.array_equal(got, want)
    assert np.array_equal(net.weights_flat, np.concatenate([a.ravel() for a in new]))
    with pytest.raises(ValueError):
        net.set_weights(new[:2])
    net.set_flat(np.arange(net.n_params))
    assert net.trainable_variables[2].tolist() == [net.n_params - 2, net.n_params - 1]
    with pytest.raises(ValueError, match="no Keras config"):
        net.to_json()


def test_mixed_templates_give_the_flat_layout_of_the_restatement():
    for name in ("rbf_then_dense", "dense_then_rbf", "rbf_wide"):
        case = rc.CASE[name]
        net = PolicyNet(case.S, case.pol_hidden, case.A, case.pol_out)
        assert (net.dims, net.acts, net.kinds, net.gammas) == (case.pol_dims, case.pol_acts, case.pol_kinds, case.pol_gammas)
        assert net.layer_slices() == rc.layer_slices(case) and net.n_params == rc.n_params(case)
        assert len(net.trainable_variables) == sum(1 if k == "rbf" else 2 for k in case.pol_kinds)
    with pytest.raises(ValueError):
        PolicyNet(4, (("dense", 8, "tanh"),), 2, "softmax")          # no RBF: that is a DenseNet
    with pytest.raises(ValueError):
        PolicyNet(4, (("rbf", 8, 0.0),), 2, "softmax")
    with pytest.raises(ValueError):
        PolicyNet(4, (("rbf", 8, float("nan")),), 2, "softmax")


def test_models_with_an_rbf_layer_are_rejected_outside_the_policy():
    net = complete_model([RBF(8, 0.5)], (4,), (2,), "softmax")
    with pytest.raises(ValueError, match="RBF"):
        SGD().compile(HyperParameters(lr=0.1, batch_size=4), net, None)
    with pytest.raises(ValueError, match="RBF"):
        BayesianModel(net)
    dt = DynamicsTraining(SGD(), {"loss": MeanSquaredError, "likelihood": "Regression"}, template=[RBF(8, 0.5)])
    with pytest.raises(ValueError, match="RBF"):
        dt._create_model((6,), (4,))


# ------------------------------------------------------------------ the C boundary
def _create_layers(dims, acts, kinds, gammas, dyn_dims=None, dyn_acts=(1, 0), K=4, H=5):
    lib = _lib.load()
    n = len(acts)
    S, A = dims[0], dims[-1]
    dyn_dims = dyn_dims or (S + A, 7, S)
    h = ctypes.c_void_p()
    i32, f32 = ctypes.c_int32, ctypes.c_float
    rc_ = lib.pyz_pilco_create_layers(n, (i32 * (n + 1))(*dims), (i32 * n)(*acts), (i32 * n)(*kinds), (f32 * n)(*gammas),
                                      len(dyn_acts), (i32 * len(dyn_dims))(*dyn_dims), (i32 * len(dyn_acts))(*dyn_acts), K, H,
                                      ctypes.byref(h))
    return rc_, h


@pytest.mark.parametrize("what, dims, acts, kinds, gammas", [
    ("an unknown kind", (4, 8, 2), (0, 4), (2, 0), (0.5, 0.0)),
    ("a negative kind", (4, 8, 2), (0, 4), (-1, 0), (0.5, 0.0)),
    ("an RBF as the last layer", (4, 8, 2), (0, 0), (1, 1), (0.5, 0.5)),
    ("an RBF as the only layer", (4, 2), (0,), (1,), (0.5,)),
    ("gamma 0", (4, 8, 2), (0, 4), (1, 0), (0.0, 0.0)),
    ("gamma < 0", (4, 8, 2), (0, 4), (1, 0), (-0.5, 0.0)),
    ("gamma NaN", (4, 8, 2), (0, 4), (1, 0), (float("nan"), 0.0)),
    ("gamma inf", (4, 8, 2), (0, 4), (1, 0), (float("inf"), 0.0)),
    ("513 RBF units", (4, 513, 2), (0, 4), (1, 0), (0.5, 0.0)),
    ("0 RBF units", (4, 0, 2), (0, 4), (1, 0), (0.5, 0.0)),
])
def test_create_layers_refuses_without_a_gpu(what, dims, acts, kinds, gammas):
    lib = _lib.load()
    code, h = _create_layers(dims, acts, kinds, gammas)
    assert code != 0 and h.value is None, what
    assert code == -1, (what, code)                 # PYZ_E_INVALID: refused by the argument check, not for want of a device
    assert lib.pyz_last_error()
    with pytest.raises(_lib.PyzError):
        _lib.check(code)


def test_act_refuses_null_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.pyz_pilco_act(None, None, None, 1, None, None) != 0 and lib.pyz_last_error()


def test_the_header_names_the_layer_kinds():
    hdr = open(os.path.join(ROOT, "include", "pyz.h")).read()
    assert "#define PYZ_PILCO_DENSE 0" in hdr and "#define PYZ_PILCO_RBF 1" in hdr
    assert _lib.PILCO_KIND == {"dense": 0, "rbf": 1}
