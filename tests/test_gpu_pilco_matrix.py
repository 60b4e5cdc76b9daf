"""Every path of the Deep-PILCO rollout kernels (csrc/pyz_pilco.h) that the sixteen cases of test_gpu_pilco.py and
test_gpu_pilco_rbf.py never took, through engine.PilcoPlan against the float64 restatement (pilco_rbf_checks.rollout,
torch CPU autograd) on the cases of tests/pilco_cases.py.  Which loop trip or branch arm each case is for is accounted
for on the CPU by tests/test_pilco_dispatch_table.py.

Bound, unchanged from test_gpu_pilco.py: cost within rtol 1e-4; states, actions (and phi, m, v after Adam steps) within
max |diff| <= 1e-4 * max |ref|; the gradient per layer slice, each against its own maximum.  The float32 restatement
sits within 1e-5 * max |ref| of the float64 one on these inputs, and every wrong oracle of pilco_cases.VARIANTS misses
the bound on every case it applies to (test_pilco_dispatch_table.py).  Every comparison prints its error over its
tolerance."""

import numpy as np
import pytest

import pilco_cases as pk
import pilco_rbf_checks as rc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPSpec, PilcoPlan

TOL = 1e-4
SENTINEL = -77.25
RUNS = [(c.name, f) for c in pk.NEW_CASES for f in c.freqs]


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_device):
    return gpu_device


class _Desc:
    """A policy description as PilcoPlan reads it."""

    def __init__(self, dims, acts, kinds, gammas):
        self.dims, self.acts, self.kinds, self.gammas = tuple(dims), tuple(acts), tuple(kinds), tuple(gammas)
        self.n_params = pk.n_params(dims, kinds)


def specs(case):
    return (_Desc(case.pol_dims, case.pol_acts, case.pol_kinds, case.pol_gammas), MLPSpec(case.dyn_dims, case.dyn_acts, "mse"))


_PLANS = {}


def plan_of(name):
    """One plan per case, shared by the tests of this module."""
    if name not in _PLANS:
        case = pk.CASE[name]
        _PLANS[name] = PilcoPlan(*specs(case), case.K, case.plan_horizon)
    return _PLANS[name]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def device_inputs(name):
    return {k: dev(v) for k, v in pk.inputs(name).items()}


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}: max |diff| {err:.3e}, max |ref| {scale:.3e}, error / tolerance {err / (TOL * scale) if scale else float('nan'):.4f}")
    assert scale > 0 and err <= TOL * scale, (what, err, scale)


def close_by_layer(case, got, ref, what):
    got = np.asarray(got)
    assert got.shape == np.asarray(ref).shape, (what, got.shape)
    for l, (sl, kind) in enumerate(zip(rc.layer_slices(case), case.pol_kinds)):
        close(got[sl], ref[sl], f"{what}, layer {l} ({kind})")


def check_rollout(case, out, ref, what):
    cost, grad, states, actions = out
    c = float(cost.cpu()[0])
    rel = abs(c - ref["cost"]) / abs(ref["cost"])
    print(f"{what}: cost {c!r} ref {ref['cost']!r}, error / tolerance {rel / TOL:.4f}")
    assert rel <= TOL
    if np.any(ref["grad"]):
        close_by_layer(case, grad.cpu().numpy(), ref["grad"], f"{what}: grad")
    else:                                                  # no step t >= 1 is counted: the cost does not depend on phi
        assert grad.shape == (len(ref["grad"]),) and not bool(grad.any()), "the gradient of an uncounted rollout is exactly 0"
    close(states.cpu().numpy(), ref["states"], f"{what}: states")
    close(actions.cpu().numpy(), ref["actions"], f"{what}: actions")
    assert states.shape[0] == case.H + 1 and actions.shape[0] == case.H


# ------------------------------------------------------------------ (1) parity and launches
@pytest.mark.parametrize("name, freq", RUNS, ids=[f"{n}-f{f}" for n, f in RUNS])
def test_rollout_matches_the_float64_restatement(name, freq):
    case = pk.CASE[name]
    _, ref = pk.reference(name, freq)
    d = device_inputs(name)
    phi0 = d["phi"].clone()
    plan = plan_of(name)
    assert plan.D_pol == rc.n_params(case) == d["phi"].numel()
    with KernelProbe(2 * case.H + 16) as kp:
        out = plan.rollout_grad(d["phi"], d["W"], d["s0"], d["eps"], case.H, pk.GAMMA, case.reward, freq=freq, use_graph=False)
    check_rollout(case, out, ref, f"{name} freq {freq}")
    assert torch.equal(d["phi"], phi0), "a gradient-only call changed phi"
    names = [n for n, _ in kp.launches]
    assert names.count("k_pilco_fwd") == case.H and names.count("k_pilco_bwd") == case.H
    assert len(names) <= 2 * case.H + 3 and all(n.startswith("k_pilco_") for n in names), sorted(set(names))


# ------------------------------------------------------------------ (2) Adam
@pytest.mark.parametrize("name", ["ks258", "pol_257", "deep8"])
def test_three_adam_steps_match_the_restatement(name):
    case = pk.CASE[name]
    inp, freq = pk.inputs(name), case.freqs[0]
    d = device_inputs(name)
    plan, lr = plan_of(name), 1e-2
    phi, m, v = d["phi"].clone(), torch.zeros_like(d["phi"]), torch.zeros_like(d["phi"])
    rphi, rm, rv = inp["phi"].copy(), np.zeros_like(inp["phi"]), np.zeros_like(inp["phi"])
    for t in (1, 2, 3):
        ref = pk.oracle(case, rphi, inp["W"], inp["s0"], inp["eps"], freq)
        cost, grad = plan.policy_step(phi, m, v, t, d["W"], d["s0"], d["eps"], case.H, pk.GAMMA, case.reward, lr=lr, freq=freq,
                                      use_graph=False)
        close_by_layer(case, grad.cpu().numpy(), ref["grad"], f"{name}: grad at t = {t}")
        rphi, rm, rv = rc.adam_step(rphi, rm, rv, ref["grad"], t, lr)
        close(phi.cpu().numpy(), rphi, f"{name}: phi after t = {t}")
        close_by_layer(case, m.cpu().numpy(), rm, f"{name}: m after t = {t}")
        close_by_layer(case, v.cpu().numpy(), rv, f"{name}: v after t = {t}")
    assert np.abs(rphi - inp["phi"]).max() > 1e-3, "the steps did not move phi: nothing was checked"


# ------------------------------------------------------------------ (3) act against the rollout
@pytest.mark.parametrize("name", ["pol_257", "deep8", "wide_softmax"])
def test_act_on_a_rollouts_states_is_its_actions_bit_for_bit(name):
    case, plan, d = pk.CASE[name], plan_of(name), device_inputs(name)
    _, _, states, actions = plan.rollout_grad(d["phi"], d["W"], d["s0"], d["eps"], case.H, pk.GAMMA, case.reward,
                                              freq=case.freqs[0], use_graph=False)
    states, actions = states.clone(), actions.clone()
    for t in range(case.H):
        got = plan.act(d["phi"], states[t])
        assert got.shape == (case.K, case.A) and torch.equal(got, actions[t]), f"act differs from the rollout at step {t}"
    flat = states[:case.H].reshape(case.H * case.K, case.S).contiguous()             # every step in one call
    assert torch.equal(plan.act(d["phi"], flat), actions.reshape(case.H * case.K, case.A))
    one = plan.act(d["phi"], states[1, case.K - 1:].contiguous())                    # N = 1
    assert one.shape == (1, case.A) and torch.equal(one, actions[1, case.K - 1:])
    assert float(actions.std()) > 0


# ------------------------------------------------------------------ (4) caller buffers
@pytest.mark.parametrize("name", ["kmax_in64", "ks258"])
def test_longer_caller_buffers_keep_their_sentinel(name):
    case, plan, d = pk.CASE[name], plan_of(name), device_inputs(name)
    _, ref = pk.reference(name)
    freq = case.freqs[0]
    f32 = dict(dtype=torch.float32, device="cuda")
    states = torch.full((case.H + 1 + 3, case.K, case.S), SENTINEL, **f32)
    actions = torch.full((case.H + 3, case.K, case.A), SENTINEL, **f32)
    args = (d["phi"], d["W"], d["s0"], d["eps"], case.H, pk.GAMMA, case.reward)
    out = plan.rollout_grad(*args, freq=freq, use_graph=False, states=states, actions=actions)
    check_rollout(case, out, ref, f"{name}, caller buffers")
    assert out[2].data_ptr() == states.data_ptr() and out[3].data_ptr() == actions.data_ptr()
    assert bool((states[case.H + 1:] == SENTINEL).all()) and bool((actions[case.H:] == SENTINEL).all())
    mine = [t.clone() for t in out]
    own = plan.rollout_grad(*args, freq=freq, use_graph=False)                         # the plan's own buffers
    check_rollout(case, own, ref, f"{name}, the plan's buffers")
    assert own[2].data_ptr() != states.data_ptr() and own[3].data_ptr() != actions.data_ptr()
    for a, b in zip(mine, own):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ (5) the graph cache
def test_five_horizon_freq_pairs_through_a_cache_of_four_graphs():
    case = pk.CASE["h257"]
    plan = PilcoPlan(*specs(case), case.K, 64)
    d = device_inputs("h257")
    inp = pk.inputs("h257")
    eps = d["eps"][:64].contiguous()
    pairs = list(pk.GRAPH_PAIRS) + [pk.GRAPH_PAIRS[0]]       # the fifth pair evicts (8, 1): the sixth call captures it again
    assert len(set(pk.GRAPH_PAIRS)) == pk.GRAPH_SLOTS + 1
    stream = torch.cuda.Stream()                             # (the legacy default stream cannot be captured)
    stream.wait_stream(torch.cuda.current_stream())

    def run(H, freq, use_graph, **buffers):
        out = plan.rollout_grad(d["phi"], d["W"], d["s0"], eps, H, pk.GAMMA, case.reward, freq=freq, use_graph=use_graph, **buffers)
        stream.synchronize()                                 # no graph is dropped while it may still be running
        return [t.clone() for t in out]

    with torch.cuda.stream(stream):
        eager = {p: run(*p, False) for p in pk.GRAPH_PAIRS}
        for H, freq in pk.GRAPH_PAIRS[:2] + pk.GRAPH_PAIRS[-1:]:      # the eager results themselves against the oracle
            ref = rc.rollout(case, inp["phi"], inp["W"], inp["s0"], inp["eps"][:H], H=H, freq=freq)
            cost, grad = eager[H, freq][:2]
            assert abs(float(cost.cpu()[0]) - ref["cost"]) <= TOL * abs(ref["cost"])
            close_by_layer(case, grad.cpu().numpy(), ref["grad"], f"H = {H}, freq = {freq}: grad")
        for p in pairs + pairs[:2]:                          # replays of (8, 1) and (9, 1) at the end
            for a, b in zip(eager[p], run(*p, True)):
                assert torch.equal(a, b), p
        # the same pairs with fresh output tensors: every pointer of the key changes, every graph is dropped
        f32 = dict(dtype=torch.float32, device="cuda")
        for p in pairs:
            states, actions = torch.zeros((65, case.K, case.S), **f32), torch.zeros((64, case.K, case.A), **f32)
            got = run(*p, True, states=states, actions=actions)
            for a, b in zip(eager[p], got):
                assert torch.equal(a, b), p
            assert torch.equal(states[:p[0] + 1], eager[p][2])
        stream.synchronize()
    assert not torch.equal(eager[8, 1][1], eager[9, 1][1])
    plan.close()


# ------------------------------------------------------------------ (6) refusals
def _no_launch(fn, exc):
    with KernelProbe(64) as kp:
        with pytest.raises(exc):
            fn()
    assert kp.launches == []


def test_refusals_come_before_any_launch():
    t, sm = "tanh", "softmax"

    def plan(pol, acts, dyn, dyn_acts, K=4, H=5):
        assert pk.admissible(K, pol, dyn, H, acts) is not None
        return PilcoPlan(_Desc(pol, acts, ("dense",) * len(acts), (0.0,) * len(acts)), MLPSpec(dyn, dyn_acts, "mse"), K, H)

    _no_launch(lambda: plan((61, 8, 4), (t, sm), (65, 16, 61), (t, "linear")), _lib.PyzError)                # S + A = 65
    _no_launch(lambda: plan((4, 513, 2), (t, sm), (6, 16, 4), (t, "linear")), _lib.PyzError)                 # width 513
    _no_launch(lambda: plan((4, 8, 2), (t, sm), (6, 513, 4), (t, "linear")), _lib.PyzError)
    _no_launch(lambda: plan((4,) + (8,) * 8 + (2,), (t,) * 8 + (sm,), (6, 16, 4), (t, "linear")), _lib.PyzError)   # 9 layers
    _no_launch(lambda: plan((4, 8, 2), (t, sm), (6,) + (16,) * 8 + (4,), (t,) * 8 + ("linear",)), _lib.PyzError)
    _no_launch(lambda: plan((4, 8, 2), (t, sm), (6, 16, 4), (t, "linear"), K=257), _lib.PyzError)
    _no_launch(lambda: plan((4, 8, 2), (t, sm), (6, 16, 4), (t, "linear"), H=4097), _lib.PyzError)
    _no_launch(lambda: plan((4, 8, 8, 2), (sm, t, sm), (6, 16, 4), (t, "linear")), _lib.PyzError)            # softmax inside
