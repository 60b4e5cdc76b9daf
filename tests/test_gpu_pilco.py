"""pyz_pilco_policy_step (csrc/pyz_pilco.h) through engine.PilcoPlan against the float64 restatement of
pilco_checks.py (torch CPU autograd), on the cases of its table.

Bound: cost within rtol 1e-4; gradient, states, actions (and phi, m, v after Adam steps) within
max |diff| <= 1e-4 * max |ref|, the project's bound for every Dense kernel (test_gpu_dense_matrix.py).  The float32
restatement sits within 1e-5 * max |ref| of the float64 one on these inputs (test_pilco_host.py), so the bound leaves the
kernels' own summation orders more than ten times that."""

import re

import numpy as np
import pytest

import pilco_checks as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPSpec, PilcoPlan

TOL = 1e-4
SENTINEL = -77.25
NAMES = [c.name for c in pc.CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_device):
    return gpu_device


def specs(case):
    return MLPSpec(case.pol_dims, case.pol_acts, "mse"), MLPSpec(case.dyn_dims, case.dyn_acts, "mse")


_PLANS = {}


def plan_of(name, extra_h=0):
    """One plan per (case, head-room), shared by the tests of this module."""
    key = (name, extra_h)
    if key not in _PLANS:
        case = pc.CASE[name]
        _PLANS[key] = PilcoPlan(*specs(case), case.K, case.H + extra_h)
    return _PLANS[key]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def device_inputs(name):
    inp, _ = pc.reference(name)
    return {k: dev(v) for k, v in inp.items()}


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}: max |diff| {err:.3e}, max |ref| {scale:.3e}, ratio {err / scale if scale else float('nan'):.3e}")
    assert scale > 0 and err <= TOL * scale, (what, err, scale)


def check_rollout(case, out, ref, H=None):
    cost, grad, states, actions = out
    H = case.H if H is None else H
    c = float(cost.cpu()[0])
    print(f"{case.name}: cost {c!r} ref {ref['cost']!r} rel {abs(c - ref['cost']) / abs(ref['cost']):.3e}")
    assert abs(c - ref["cost"]) <= TOL * abs(ref["cost"])
    close(grad.cpu().numpy(), ref["grad"], "grad")
    close(states.cpu().numpy(), ref["states"], "states")
    close(actions.cpu().numpy(), ref["actions"], "actions")
    assert states.shape[0] == H + 1 and actions.shape[0] == H


# ------------------------------------------------------------------ (1) parity
@pytest.mark.parametrize("name", NAMES)
def test_rollout_matches_the_float64_restatement(name):
    case = pc.CASE[name]
    _, ref = pc.reference(name)
    d = device_inputs(name)
    phi0 = d["phi"].clone()
    out = plan_of(name).rollout_grad(d["phi"], d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward, use_graph=False)
    check_rollout(case, out, ref)
    assert torch.equal(d["phi"], phi0), "a gradient-only call changed phi"


# ------------------------------------------------------------------ (2) Adam
@pytest.mark.parametrize("name", ["cart_softmax", "odd"])
def test_three_adam_steps_match_the_restatement(name):
    case = pc.CASE[name]
    inp, _ = pc.reference(name)
    d = device_inputs(name)
    plan, lr = plan_of(name), 1e-2
    phi, m, v = d["phi"].clone(), torch.zeros_like(d["phi"]), torch.zeros_like(d["phi"])
    rphi, rm, rv = inp["phi"].copy(), np.zeros_like(inp["phi"]), np.zeros_like(inp["phi"])
    for t in (1, 2, 3):
        ref = pc.rollout(case, rphi, inp["W"], inp["s0"], inp["eps"])
        cost, grad = plan.policy_step(phi, m, v, t, d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward, lr=lr,
                                      use_graph=False)
        close(grad.cpu().numpy(), ref["grad"], f"grad at t = {t}")
        rphi, rm, rv = pc.adam_step(rphi, rm, rv, ref["grad"], t, lr)
        close(phi.cpu().numpy(), rphi, f"phi after t = {t}")
        close(m.cpu().numpy(), rm, f"m after t = {t}")
        close(v.cpu().numpy(), rv, f"v after t = {t}")
    assert np.abs(rphi - inp["phi"]).max() > 1e-3, "the steps did not move phi: nothing was checked"


def test_gradient_only_leaves_phi_and_the_moments_bit_identical():
    name = "cart_softmax"
    case = pc.CASE[name]
    d = device_inputs(name)
    phi = d["phi"].clone()
    m, v = torch.full_like(phi, 0.25), torch.full_like(phi, 0.5)
    keep = [t.clone() for t in (phi, m, v)]
    plan_of(name).policy_step(phi, m, v, 0, d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward, lr=1e-2, use_graph=False)
    torch.cuda.synchronize()
    for got, want in zip((phi, m, v), keep):
        assert torch.equal(got, want)


# ------------------------------------------------------------------ (3) reproducibility
@pytest.mark.parametrize("name", ["odd", "example"])
def test_same_bits_from_call_to_call_and_from_the_graph(name):
    case = pc.CASE[name]
    _, ref = pc.reference(name)
    d = device_inputs(name)
    plan = plan_of(name)
    args = (d["phi"], d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward)
    runs = []
    stream = torch.cuda.Stream()          # (the legacy default stream cannot be captured)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for use_graph in (False, False, True, True):       # the second graph call replays what the first captured
            out = plan.rollout_grad(*args, use_graph=use_graph)
            runs.append([t.clone() for t in out])
        stream.synchronize()
    check_rollout(case, runs[2], ref)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    # an Adam step through the graph, twice from the same start: the scalars of a call are not baked into the graph
    got = []
    with torch.cuda.stream(stream):
        phi, m, v = d["phi"].clone(), torch.zeros_like(d["phi"]), torch.zeros_like(d["phi"])
        for use_graph in (False, True):
            phi.copy_(d["phi"]), m.zero_(), v.zero_()
            for t in (1, 2):
                plan.policy_step(phi, m, v, t, d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward, lr=1e-2,
                                 use_graph=use_graph)
            got.append([x.clone() for x in (phi, m, v)])
        stream.synchronize()
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert not torch.equal(got[0][0], d["phi"])


# ------------------------------------------------------------------ (4) launch count
@pytest.mark.parametrize("name", ["min", "freq2"])
def test_a_rollout_is_2h_plus_3_launches_of_this_library(name):
    case = pc.CASE[name]
    d = device_inputs(name)
    plan = plan_of(name)
    with KernelProbe(4 * case.H + 16) as kp:
        plan.rollout_grad(d["phi"], d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward, use_graph=False)
    names = [n for n, _ in kp.launches]
    assert names.count("k_pilco_fwd") == case.H and names.count("k_pilco_bwd") == case.H
    rest = [n for n in names if n not in ("k_pilco_fwd", "k_pilco_bwd")]
    assert len(rest) <= 3 and all(n.startswith("k_pilco_") for n in rest), rest
    assert len(names) == 2 * case.H + len(rest)


# ------------------------------------------------------------------ (5) buffer edges
@pytest.mark.parametrize("name", ["acb_two_hidden", "odd"])
def test_longer_buffers_keep_their_sentinel_and_a_shorter_horizon_matches(name):
    case = pc.CASE[name]
    inp, ref = pc.reference(name)
    d = device_inputs(name)
    plan = plan_of(name, extra_h=3)                        # max_horizon three steps past the horizon used
    f32 = dict(dtype=torch.float32, device="cuda")
    eps = torch.full((case.H + 3, case.K, case.S), float("nan"), **f32)     # a step past H must not be read either
    eps[:case.H] = d["eps"]
    states = torch.full((case.H + 1 + 3, case.K, case.S), SENTINEL, **f32)
    actions = torch.full((case.H + 3, case.K, case.A), SENTINEL, **f32)
    out = plan.rollout_grad(d["phi"], d["W"], d["s0"], eps, case.H, pc.GAMMA, case.reward, use_graph=False, states=states,
                            actions=actions)
    check_rollout(case, out, ref)
    assert out[2].data_ptr() == states.data_ptr() and out[3].data_ptr() == actions.data_ptr()
    assert bool((states[case.H + 1:] == SENTINEL).all()) and bool((actions[case.H:] == SENTINEL).all())
    # the same plan at a shorter horizon (its own freq): the tape of the longer call must not leak into it
    H2 = case.H - 5
    ref2 = pc.rollout(case, inp["phi"], inp["W"], inp["s0"], inp["eps"][:H2], H=H2)
    states.fill_(SENTINEL), actions.fill_(SENTINEL)
    out2 = plan.rollout_grad(d["phi"], d["W"], d["s0"], eps, H2, pc.GAMMA, case.reward, use_graph=False, states=states,
                             actions=actions)
    check_rollout(case, out2, ref2, H=H2)
    assert bool((states[H2 + 1:] == SENTINEL).all()) and bool((actions[H2:] == SENTINEL).all())


# ------------------------------------------------------------------ (6) refusals
def _no_launch(fn, exc):
    with KernelProbe(64) as kp:
        with pytest.raises(exc):
            fn()
    assert kp.launches == []


def test_refusals_come_before_any_launch():
    case = pc.CASE["cart_softmax"]
    pol, dyn = specs(case)
    d = device_inputs("cart_softmax")
    _no_launch(lambda: PilcoPlan(pol, dyn, 1, case.H), _lib.PyzError)                       # K = 1
    bad_dyn = MLPSpec(case.dyn_dims, ("relu", "tanh"), "mse")
    _no_launch(lambda: PilcoPlan(pol, bad_dyn, case.K, case.H), _lib.PyzError)              # non-linear dynamics output
    wrong_in = MLPSpec((case.S + case.A + 1, 16, case.S), ("relu", "linear"), "mse")
    _no_launch(lambda: PilcoPlan(pol, wrong_in, case.K, case.H), _lib.PyzError)             # dims that do not fit
    _no_launch(lambda: PilcoPlan(pol, dyn, 257, case.H), _lib.PyzError)                     # past the limits
    plan = plan_of("cart_softmax")
    args = dict(phi=d["phi"], W=d["W"], s0=d["s0"], eps=d["eps"], horizon=case.H, gamma=pc.GAMMA, reward=case.reward,
                use_graph=False)
    _no_launch(lambda: plan.rollout_grad(**{**args, "reward": "Acb 2 factors"}), _lib.PyzError)   # S = 4 < 5
    _no_launch(lambda: plan.rollout_grad(**{**args, "reward": "Nope"}), ValueError)
    _no_launch(lambda: plan.rollout_grad(**{**args, "phi": d["phi"].double()}), TypeError)
    _no_launch(lambda: plan.rollout_grad(**{**args, "phi": d["phi"].cpu()}), TypeError)
    _no_launch(lambda: plan.rollout_grad(**{**args, "W": d["W"][:-1].contiguous()}), ValueError)
    _no_launch(lambda: plan.rollout_grad(**{**args, "s0": d["s0"].t().contiguous()}), ValueError)
    _no_launch(lambda: plan.rollout_grad(**{**args, "eps": d["eps"][:-1].contiguous()}), ValueError)
    _no_launch(lambda: plan.rollout_grad(**{**args, "horizon": case.H + 1}), ValueError)
    _no_launch(lambda: plan.rollout_grad(**{**args, "states": torch.zeros(case.H, case.K, case.S, device="cuda")}), ValueError)
    # the C entry point's own checks, with Python's out of the way
    lib, C = _lib.load(), __import__("ctypes")
    one, grad = torch.zeros(1, device="cuda"), torch.zeros_like(d["phi"])

    def raw(H=case.H, freq=1, reward=0, t=0, phi=d["phi"]):
        _lib.check(lib.pyz_pilco_policy_step(plan.h, _lib.ptr(phi), None, None, t, _lib.ptr(d["W"]), _lib.ptr(d["s0"]),
                                             _lib.ptr(d["eps"]), H, freq, 0.95, reward, 0.0, _lib.ptr(one), _lib.ptr(grad),
                                             None, None, 0, None))
    for kw in (dict(H=0), dict(H=case.H + 1), dict(freq=0), dict(reward=1), dict(reward=2), dict(t=1), dict(phi=None)):
        _no_launch(lambda: raw(**kw), _lib.PyzError)


# ------------------------------------------------------------------ (7) end to end
def test_bayesian_dynamics_learns_on_the_built_in_cartpole(tmp_path, monkeypatch):
    from bayesian_inference_for_nn_amd.dynamics import BayesianDynamics, DynamicsTraining, NNPolicy, envs
    from bayesian_inference_for_nn_amd.losses import MeanSquaredError
    from bayesian_inference_for_nn_amd.optimizers import SWAG
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

    K, H = 8, 10
    dt = DynamicsTraining(SWAG(), {"loss": MeanSquaredError, "likelihood": "Regression"}, template=[(16, "relu")],
                          hyperparams=HyperParameters(lr=1e-2, batch_size=8, k=4, scale=1.0, frequency=1))
    policy = NNPolicy([(8, "tanh")], HyperParameters(lr=1e-2))
    bd = BayesianDynamics(envs.CartPole(seed=0), H, dt, policy, "Cart", (30, K, 0.95), seed=5)
    dt.compile_more({"starting_model": dt.model, "seed": 1})

    calls, phis = [], [policy.network.weights_flat.copy()]
    inner = PilcoPlan.policy_step

    def spy(self, phi, m, v, t, W, s0, eps, horizon, gamma, reward, **kw):
        before = [x.clone() for x in (phi, m, v, W, s0, eps)]
        out = inner(self, phi, m, v, t, W, s0, eps, horizon, gamma, reward, **kw)
        torch.cuda.synchronize()
        calls.append(dict(before=before, t=t, H=horizon, gamma=gamma, reward=reward, kw=kw, cost=float(out[0].item()),
                          grad=out[1].cpu().numpy().copy(), phi=phi.cpu().numpy().copy()))
        return out
    monkeypatch.setattr(PilcoPlan, "policy_step", spy)

    record = tmp_path / "record.txt"
    real_train = dt._train

    def train_and_note(*a):
        real_train(*a)
        phis.append(policy.network.weights_flat.copy())       # the policy as it stands when an epoch's trial is done
    dt._train = train_and_note
    bd.learn(3, str(record), 1)
    phis.append(policy.network.weights_flat.copy())

    text = record.read_text()
    assert re.findall(r"^Learning epoch (\d+)$", text, flags=re.M) == ["2", "3"]
    assert len(re.findall(r"^Total cost: -?\d", text, flags=re.M)) == 2
    assert len(re.findall(r"^Gradient sample: \[.*\], length 4$", text, flags=re.M)) == 2
    assert text.count("; Actions hor: ") == 2
    # phis: initial, after the trainings of epochs 1, 2, 3, at the end.  The policy moves in the updates of epochs 2 and 3 only
    assert np.array_equal(phis[0], phis[1]) and np.array_equal(phis[1], phis[2])
    assert not np.array_equal(phis[2], phis[3]) and not np.array_equal(phis[3], phis[4])
    assert [c["t"] for c in calls] == [1, 2] and len(dt.features) == 3 * H
    assert all(c["H"] == H and c["reward"] == "Cart" and c["kw"]["freq"] == 1 and c["kw"]["lr"] == 1e-2 for c in calls)

    # the second update against the restatement, on the inputs the plan was given
    c = calls[1]
    phi, m, v, W, s0, eps = (x.cpu().numpy().astype(np.float64) for x in c["before"])
    case = pc.Case("e2e", 4, 2, K, H, (8,), "tanh", "softmax", (16,), "relu", "Cart")
    ref = pc.rollout(case, phi, W, s0, eps, gamma=0.95)
    assert ref["min_sd"] > 0 and abs(c["cost"] - ref["cost"]) <= TOL * abs(ref["cost"])
    close(c["grad"], ref["grad"], "grad of the captured update")
    close(c["phi"], pc.adam_step(phi, m, v, ref["grad"], 2, 1e-2)[0], "phi after the captured update")
    assert np.array_equal(c["phi"].astype(np.float32), phis[4])
    assert np.abs(eps).max() > 1.0 and abs(eps.mean()) < 0.2 and not np.array_equal(eps, calls[0]["before"][5].cpu().numpy())
