"""The RBF policy layer of the Deep-PILCO kernels (csrc/pyz_pilco.h: pilco_rbf, pilco_rbf_dx, k_pilco_act) through
engine.PilcoPlan against the float64 restatement of pilco_rbf_checks.py (torch CPU autograd), on the cases of its table.

Bound, as in test_gpu_pilco.py: cost within rtol 1e-4; states, actions (and phi, m, v after Adam steps) within
max |diff| <= 1e-4 * max |ref|.  The gradient is compared per layer slice, each against its own maximum: a wrong
gradient of the RBF means must not hide under a larger Dense gradient.  The float32 restatement sits within
1e-5 * max |ref| of the float64 one on these inputs, per slice too (test_pilco_rbf_host.py)."""

import ctypes as C
import re

import numpy as np
import pytest

import pilco_checks as pc
import pilco_rbf_checks as rc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPSpec, PilcoPlan
from bayesian_inference_for_nn_amd.nn.model import PolicyNet

TOL = 1e-4
SENTINEL = -77.25
NAMES = [c.name for c in rc.CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_device):
    return gpu_device


def specs(case):
    """(policy description, dynamics spec) of a case of either table."""
    dyn = MLPSpec(case.dyn_dims, case.dyn_acts, "mse")
    if isinstance(case, pc.Case):
        return MLPSpec(case.pol_dims, case.pol_acts, "mse"), dyn
    return PolicyNet(case.S, case.pol_hidden, case.A, case.pol_out), dyn


_PLANS = {}


def plan_of(name, extra_h=0):
    """One plan per (case, head-room), shared by the tests of this module."""
    key = (name, extra_h)
    if key not in _PLANS:
        case = rc.CASE[name]
        _PLANS[key] = PilcoPlan(*specs(case), case.K, case.H + extra_h)
    return _PLANS[key]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def device_inputs(name):
    inp, _ = rc.reference(name)
    return {k: dev(v) for k, v in inp.items()}


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}: max |diff| {err:.3e}, max |ref| {scale:.3e}, ratio {err / scale if scale else float('nan'):.3e}")
    assert scale > 0 and err <= TOL * scale, (what, err, scale)


def close_by_layer(case, got, ref, what):
    got = np.asarray(got)
    assert got.shape == np.asarray(ref).shape, (what, got.shape)
    for l, (sl, kind) in enumerate(zip(rc.layer_slices(case), case.pol_kinds)):
        close(got[sl], ref[sl], f"{what}, layer {l} ({kind})")


def check_rollout(case, out, ref, H=None):
    cost, grad, states, actions = out
    H = case.H if H is None else H
    c = float(cost.cpu()[0])
    print(f"{case.name}: cost {c!r} ref {ref['cost']!r} rel {abs(c - ref['cost']) / abs(ref['cost']):.3e}")
    assert abs(c - ref["cost"]) <= TOL * abs(ref["cost"])
    close_by_layer(case, grad.cpu().numpy(), ref["grad"], "grad")
    close(states.cpu().numpy(), ref["states"], "states")
    close(actions.cpu().numpy(), ref["actions"], "actions")
    assert states.shape[0] == H + 1 and actions.shape[0] == H


# ------------------------------------------------------------------ (1) parity
@pytest.mark.parametrize("name", NAMES)
def test_rollout_matches_the_float64_restatement(name):
    case = rc.CASE[name]
    _, ref = rc.reference(name)
    d = device_inputs(name)
    phi0 = d["phi"].clone()
    plan = plan_of(name)
    assert plan.D_pol == rc.n_params(case) == d["phi"].numel()
    out = plan.rollout_grad(d["phi"], d["W"], d["s0"], d["eps"], case.H, rc.GAMMA, case.reward, use_graph=False)
    check_rollout(case, out, ref)
    assert torch.equal(d["phi"], phi0), "a gradient-only call changed phi"


# ------------------------------------------------------------------ (2) Adam
@pytest.mark.parametrize("name", ["rbf_cart", "rbf_odd"])
def test_three_adam_steps_match_the_restatement(name):
    case = rc.CASE[name]
    inp, _ = rc.reference(name)
    d = device_inputs(name)
    plan, lr = plan_of(name), 1e-2
    phi, m, v = d["phi"].clone(), torch.zeros_like(d["phi"]), torch.zeros_like(d["phi"])
    rphi, rm, rv = inp["phi"].copy(), np.zeros_like(inp["phi"]), np.zeros_like(inp["phi"])
    for t in (1, 2, 3):
        ref = rc.rollout(case, rphi, inp["W"], inp["s0"], inp["eps"])
        cost, grad = plan.policy_step(phi, m, v, t, d["W"], d["s0"], d["eps"], case.H, rc.GAMMA, case.reward, lr=lr,
                                      use_graph=False)
        close_by_layer(case, grad.cpu().numpy(), ref["grad"], f"grad at t = {t}")
        rphi, rm, rv = rc.adam_step(rphi, rm, rv, ref["grad"], t, lr)
        close(phi.cpu().numpy(), rphi, f"phi after t = {t}")
        close_by_layer(case, m.cpu().numpy(), rm, f"m after t = {t}")
        close_by_layer(case, v.cpu().numpy(), rv, f"v after t = {t}")
    mean = rc.layer_slices(case)[0]
    assert np.abs(rphi - inp["phi"])[mean].max() > 1e-3, "the steps did not move the RBF means: nothing was checked"


# ------------------------------------------------------------------ (3) reproducibility
@pytest.mark.parametrize("name", ["rbf_odd", "rbf_example"])
def test_same_bits_from_call_to_call_and_from_the_graph(name):
    case = rc.CASE[name]
    _, ref = rc.reference(name)
    d = device_inputs(name)
    plan = plan_of(name)
    args = (d["phi"], d["W"], d["s0"], d["eps"], case.H, rc.GAMMA, case.reward)
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
                plan.policy_step(phi, m, v, t, d["W"], d["s0"], d["eps"], case.H, rc.GAMMA, case.reward, lr=1e-2,
                                 use_graph=use_graph)
            got.append([x.clone() for x in (phi, m, v)])
        stream.synchronize()
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert not torch.equal(got[0][0], d["phi"])


# ------------------------------------------------------------------ (4) launch count
def test_a_rollout_is_2h_plus_3_launches_of_this_library():
    name = "rbf_min"
    case = rc.CASE[name]
    d = device_inputs(name)
    plan = plan_of(name)
    with KernelProbe(4 * case.H + 16) as kp:
        plan.rollout_grad(d["phi"], d["W"], d["s0"], d["eps"], case.H, rc.GAMMA, case.reward, use_graph=False)
    names = [n for n, _ in kp.launches]
    assert names.count("k_pilco_fwd") == case.H and names.count("k_pilco_bwd") == case.H
    assert len(names) == 2 * case.H + 3 and all(n.startswith("k_pilco_") for n in names), names
    with KernelProbe(8) as kp:
        plan.act(d["phi"], d["s0"])
    assert [n for n, _ in kp.launches] == ["k_pilco_act"]


# ------------------------------------------------------------------ (5) buffer edges
def test_longer_buffers_keep_their_sentinel_and_a_shorter_horizon_matches():
    name = "rbf_odd"
    case = rc.CASE[name]
    inp, ref = rc.reference(name)
    d = device_inputs(name)
    plan = plan_of(name, extra_h=3)                        # max_horizon three steps past the horizon used
    f32 = dict(dtype=torch.float32, device="cuda")
    eps = torch.full((case.H + 3, case.K, case.S), float("nan"), **f32)     # a step past H must not be read either
    eps[:case.H] = d["eps"]
    states = torch.full((case.H + 1 + 3, case.K, case.S), SENTINEL, **f32)
    actions = torch.full((case.H + 3, case.K, case.A), SENTINEL, **f32)
    out = plan.rollout_grad(d["phi"], d["W"], d["s0"], eps, case.H, rc.GAMMA, case.reward, use_graph=False, states=states,
                            actions=actions)
    check_rollout(case, out, ref)
    assert out[2].data_ptr() == states.data_ptr() and out[3].data_ptr() == actions.data_ptr()
    assert bool((states[case.H + 1:] == SENTINEL).all()) and bool((actions[case.H:] == SENTINEL).all())
    # the same plan at a shorter horizon (its own freq): the tape of the longer call must not leak into it
    H2 = case.H - 5
    ref2 = rc.rollout(case, inp["phi"], inp["W"], inp["s0"], inp["eps"][:H2], H=H2)
    states.fill_(SENTINEL), actions.fill_(SENTINEL)
    out2 = plan.rollout_grad(d["phi"], d["W"], d["s0"], eps, H2, rc.GAMMA, case.reward, use_graph=False, states=states,
                             actions=actions)
    check_rollout(case, out2, ref2, H=H2)
    assert bool((states[H2 + 1:] == SENTINEL).all()) and bool((actions[H2:] == SENTINEL).all())


# ------------------------------------------------------------------ (6), (7) act against the rollout
def _act_equals_the_rollouts_actions(case, plan, d):
    cost, grad, states, actions = plan.rollout_grad(d["phi"], d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward,
                                                    use_graph=False)
    states, actions = states.clone(), actions.clone()
    guard = 3                                              # rows past the N asked for keep their sentinel
    for t in sorted({0, case.H // 2, case.H - 1}):
        got = plan.act(d["phi"], states[t])
        assert got.shape == (case.K, case.A) and torch.equal(got, actions[t]), f"act differs from the rollout at step {t}"
    # every step in one call: N = H * K rows, more than one workgroup per particle count
    flat = states[:case.H].reshape(case.H * case.K, case.S).contiguous()
    assert torch.equal(plan.act(d["phi"], flat), actions.reshape(case.H * case.K, case.A))
    # the C entry with a longer output buffer: exactly N rows are written
    out = torch.full((case.K + guard, case.A), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(plan.lib.pyz_pilco_act(plan.h, _lib.ptr(d["phi"]), _lib.ptr(states[0]), case.K, _lib.ptr(out), None))
    torch.cuda.synchronize()
    assert torch.equal(out[:case.K], actions[0]) and bool((out[case.K:] == SENTINEL).all())
    one = plan.act(d["phi"], states[1, :1].contiguous())                       # N = 1
    assert torch.equal(one, actions[1, :1])


@pytest.mark.parametrize("name", ["rbf_odd", "dense_then_rbf"])
def test_act_on_a_rollouts_states_is_its_actions_bit_for_bit(name):
    _act_equals_the_rollouts_actions(rc.CASE[name], plan_of(name), device_inputs(name))


def test_act_for_a_dense_only_policy_is_the_rollouts_actions_bit_for_bit():
    case = pc.CASE["cart_softmax"]
    inp, _ = pc.reference("cart_softmax")
    plan = PilcoPlan(*specs(case), case.K, case.H)
    _act_equals_the_rollouts_actions(case, plan, {k: dev(v) for k, v in inp.items()})


# ------------------------------------------------------------------ (8) old entry against new entry
class _Desc:
    """A policy description as PilcoPlan reads it."""

    def __init__(self, dims, acts, kinds, gammas, n_params=1):
        self.dims, self.acts, self.kinds, self.gammas, self.n_params = dims, acts, kinds, gammas, n_params


def test_a_dense_plan_through_create_layers_is_bit_identical_to_one_through_create():
    case = pc.CASE["odd"]
    inp, ref = pc.reference("odd")
    d = {k: dev(v) for k, v in inp.items()}
    pol, dyn = specs(case)
    old = PilcoPlan(pol, dyn, case.K, case.H)
    n = len(case.pol_acts)                                 # a description with kinds: PilcoPlan takes pyz_pilco_create_layers
    new = PilcoPlan(_Desc(case.pol_dims, case.pol_acts, ("dense",) * n, (0.0,) * n, pol.n_params), dyn, case.K, case.H)
    assert new.workspace_bytes == old.workspace_bytes
    outs = []
    for plan in (old, new):
        phi, m, v = d["phi"].clone(), torch.zeros_like(d["phi"]), torch.zeros_like(d["phi"])
        res = plan._call(phi, m, v, 1, d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward, 1e-2, None, False, None, None)
        outs.append([x.clone() for x in res] + [phi, m, v])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    close(outs[1][1].cpu().numpy(), ref["grad"], "grad through pyz_pilco_create_layers")


# ------------------------------------------------------------------ (9) refusals
def _no_launch(fn, exc):
    with KernelProbe(64) as kp:
        with pytest.raises(exc):
            fn()
    assert kp.launches == []


def test_refusals_come_before_any_launch():
    case = rc.CASE["rbf_cart"]
    pol, dyn = specs(case)
    d = device_inputs("rbf_cart")
    lin, sm = "linear", "softmax"
    for desc in (_Desc((4, 8, 2), (lin, lin), ("rbf", "rbf"), (0.5, 0.5)),               # an RBF as the last layer
                 _Desc((4, 8, 2), (lin, sm), ("rbf", "dense"), (0.0, 0.0)),              # gamma 0
                 _Desc((4, 8, 2), (lin, sm), ("rbf", "dense"), (float("nan"), 0.0)),
                 _Desc((4, 8, 2), (lin, sm), ("rbf", "dense"), (float("inf"), 0.0)),
                 _Desc((4, 8, 2), (lin, sm), ("rbf", "dense"), (-1.0, 0.0)),
                 _Desc((4, 513, 2), (lin, sm), ("rbf", "dense"), (0.5, 0.0)),            # past the width limit
                 _Desc((4, 8, 2), ("tanh", sm), ("rbf", "dense"), (0.5, 0.0))):          # an RBF takes no activation
        _no_launch(lambda: PilcoPlan(desc, dyn, case.K, case.H), _lib.PyzError)
    _no_launch(lambda: PilcoPlan(pol, dyn, 1, case.H), _lib.PyzError)                       # K = 1, as for a Dense policy
    # an unknown kind, with Python's name table out of the way
    lib, n = _lib.load(), 2
    i32 = C.c_int32
    h = C.c_void_p()

    def raw_create():
        _lib.check(lib.pyz_pilco_create_layers(n, (i32 * 3)(4, 8, 2), (i32 * 2)(0, 4), (i32 * 2)(7, 0), (C.c_float * 2)(0.5, 0.0),
                                               2, (i32 * 3)(6, 16, 4), (i32 * 2)(1, 0), case.K, case.H, C.byref(h)))
    _no_launch(raw_create, _lib.PyzError)
    assert h.value is None
    # act
    plan = plan_of("rbf_cart")
    _no_launch(lambda: plan.act(d["phi"], d["s0"][:0]), ValueError)                          # N = 0
    _no_launch(lambda: plan.act(d["phi"], d["s0"][:, :3].contiguous()), ValueError)
    _no_launch(lambda: plan.act(d["phi"][:-1].contiguous(), d["s0"]), ValueError)
    _no_launch(lambda: plan.act(d["phi"].double(), d["s0"]), TypeError)
    _no_launch(lambda: plan.act(d["phi"], d["s0"].cpu()), TypeError)
    out = torch.zeros(case.K, case.A, device="cuda")
    p = _lib.ptr
    for args in ((None, p(d["phi"]), p(d["s0"]), case.K, p(out)), (plan.h, None, p(d["s0"]), case.K, p(out)),
                 (plan.h, p(d["phi"]), None, case.K, p(out)), (plan.h, p(d["phi"]), p(d["s0"]), case.K, None),
                 (plan.h, p(d["phi"]), p(d["s0"]), 0, p(out)), (plan.h, p(d["phi"]), p(d["s0"]), -3, p(out))):
        _no_launch(lambda: _lib.check(lib.pyz_pilco_act(*args, None)), _lib.PyzError)


# ------------------------------------------------------------------ (10) end to end
def test_bayesian_dynamics_learns_an_rbf_policy_on_the_built_in_cartpole(tmp_path, monkeypatch):
    from bayesian_inference_for_nn_amd.dynamics import RBF, BayesianDynamics, DynamicsTraining, NNPolicy, envs
    from bayesian_inference_for_nn_amd.losses import MeanSquaredError
    from bayesian_inference_for_nn_amd.optimizers import SWAG
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

    K, H = 8, 10
    dt = DynamicsTraining(SWAG(), {"loss": MeanSquaredError, "likelihood": "Regression"}, template=[(16, "relu")],
                          hyperparams=HyperParameters(lr=1e-2, batch_size=8, k=4, scale=1.0, frequency=1))
    policy = NNPolicy([RBF(8, 0.5)], HyperParameters(lr=1e-2))
    bd = BayesianDynamics(envs.CartPole(seed=0), H, dt, policy, "Cart", (30, K, 0.95), seed=5)
    dt.compile_more({"starting_model": dt.model, "seed": 1})
    assert isinstance(policy.network, PolicyNet) and policy.network.dims == (4, 8, 2)

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
    assert len(re.findall(r"^Gradient sample: \[.*\], length 3$", text, flags=re.M)) == 2
    # phis: initial, after the trainings of epochs 1, 2, 3, at the end.  The policy moves in the updates of epochs 2 and 3 only
    assert np.array_equal(phis[0], phis[1]) and np.array_equal(phis[1], phis[2])
    assert not np.array_equal(phis[2], phis[3]) and not np.array_equal(phis[3], phis[4])
    assert not np.array_equal(phis[2][:32], phis[4][:32]), "the RBF means did not move"
    assert [c["t"] for c in calls] == [1, 2] and len(dt.features) == 3 * H
    assert all(c["H"] == H and c["reward"] == "Cart" and c["kw"]["freq"] == 1 and c["kw"]["lr"] == 1e-2 for c in calls)
    # the trial of epoch 3 drove the cart through NNPolicy.act, the policy forward on the device
    assert len(bd.last_takes) == H and all(int(a) in (0, 1) for a in bd.last_takes)

    # the second update against the restatement, on the inputs the plan was given
    c = calls[1]
    phi, m, v, W, s0, eps = (x.cpu().numpy().astype(np.float64) for x in c["before"])
    case = rc.Case("e2e", 4, 2, K, H, (("rbf", 8, 0.5),), "softmax", (16,), "relu", "Cart")
    ref = rc.rollout(case, phi, W, s0, eps, gamma=0.95)
    assert ref["min_sd"] > 0 and abs(c["cost"] - ref["cost"]) <= TOL * abs(ref["cost"])
    close_by_layer(case, c["grad"], ref["grad"], "grad of the captured update")
    close(c["phi"], rc.adam_step(phi, m, v, ref["grad"], 2, 1e-2)[0], "phi after the captured update")
    assert np.array_equal(c["phi"].astype(np.float32), phis[4])
