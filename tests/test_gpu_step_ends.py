"""The serial head and tail of the step kernels, on the GPU: the cross-wave combine of the Dense tile kernels with every wave
count, bit for bit against its host restatement on inputs that tell the orders apart (tests/combine_cases.py), and
device-resident runs of a two-layer and a three-layer model (layer selection of k_wgrad_all, odd batches, a ragged last
batch, every update mode) against the same steps as single *_step calls, bit for bit.

The ragged case: its last step has 7 rows while the run launches every step for its largest batch, 33.  The wave count of
k_wgrad_all follows the LAUNCH batch (pyz_pick_waves: 17 reduction steps -> S = 2, 4 steps -> S = 1), so the run adds that
step's batch rows in another association than the single step does: those two can only agree to rounding, as
tests/test_gpu_run_matrix.py documents for its ragged chains.  The comparison bit for bit therefore ends in front of that
step for the single steps; the ragged step itself is held bit for bit against the eager-chained run (the same launches
without a graph) and to 2e-6 of the largest magnitude against the single steps, the bound of that matrix.  Measured on the
three-layer case: at most 3.0e-8 in theta (magnitudes of order 1), 3.7e-9 in mean, 1.2e-10 in sq_mean."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import combine_cases as cc  # noqa: E402
import dense_cases as dc  # noqa: E402
import run_cases as rc  # noqa: E402
from run_cases import RunCall, RunCase  # noqa: E402
from test_gpu_run_matrix import Dev, assert_same, dev, probed, same_bits, written_slots  # noqa: E402


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in rc.ENV_FORBIDDEN if os.environ.get(k)]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the expected launches of this module assume their defaults")
    from bayesian_inference_for_nn_amd import engine
    return engine


# ---------------------------------------------------------------- forward combine
@pytest.mark.parametrize("name,batch,n,k", cc.FORWARD_CASES, ids=[c[0] for c in cc.FORWARD_CASES])
def test_forward_combine_adds_the_waves_in_order(eng, name, batch, n, k):
    S = cc.waves_of(batch, n, k)
    a, w, bias = cc.forward_inputs(batch, n, k, S)
    want = cc.host_forward(a, w, bias, S)
    plan = eng.MLPPlan(eng.MLPSpec((k, n), ("linear",), "mse"), max_batch=batch)
    theta = dev(np.concatenate([w.reshape(-1), bias]))
    x = dev(a)
    with eng.KernelProbe(8) as kp:
        got = plan.forward(theta, x)
    torch.cuda.synchronize()
    assert [rc._norm(nm) for nm, _ in kp.launches].count("k_dense_fwd") == 1
    got = got.cpu().numpy().reshape(batch, n)
    plan.close()
    bad = np.flatnonzero(got.view(np.int32).reshape(-1) != want.view(np.int32).reshape(-1))
    if bad.size:
        i = bad[0]
        others = {o.__name__: cc.host_forward(a, w, bias, S, o).reshape(-1)[i] for o in (cc.combine_pairwise, cc.combine_reversed)}
        pytest.fail(f"{name}: S = {S}, {bad.size} of {want.size} elements differ; element {divmod(int(i), n)}: got {got.reshape(-1)[i]!r}, in order {want.reshape(-1)[i]!r}, {others}")


# ---------------------------------------------------------------- resident runs
T, R, SM = "tanh", "relu", "softmax"
RUN_CASES = [
    # (case, batch sizes of an n-step run)
    (RunCase("ends_l2_b70", (20, 12, 3), (T, SM), "scce", 70, (70,) * rc.N_STEPS, swag=(3, 2)), lambda n: (70,) * n),
    (RunCase("ends_l3_b33_ragged7", (9, 40, 33, 3), (T, R, SM), "scce", 33, (33,) * rc.N_STEPS, swag=(3, 2), bbb_lr=0.25),
     lambda n: (33,) * (n - 1) + (7,)),
]
_DATA = {}


def data_of(case):
    if case.name not in _DATA:
        _DATA[case.name] = rc.run_data(case, slots=48)
    return _DATA[case.name]


def call_of(case, mode, sizes):
    lr = (case.bbb_lr if mode == "bbb" else case.lr) / 8
    k, freq = case.swag if mode == "swag" else (0, 0)
    return RunCall(case.n0, case.slot0, tuple(sizes), tuple(lr * (1.0 - (i % 8) / 16.0) for i in range(len(sizes))), k, freq, False)


def test_shapes_reach_what_they_are_for():
    (two, _), (three, _) = RUN_CASES
    assert two.fused and three.fused and len(three.dims) - 1 == 3
    assert rc.wgrad_tile_count(three.dims) == 8 and [dc.wgrad_tiles(K, N) for K, N in zip(three.dims[:-1], three.dims[1:])] == [2, 4, 2]
    assert two.bmax % 2 == 0 and three.bmax % 2 == 1                                   # the peeled row of an odd batch
    assert three.S == 2 and dc.pick_waves(8, dc.wgrad_steps(7))[0] == 1                  # (see the module's docstring)
    assert two.S == dc.pick_waves(rc.wgrad_tile_count(two.dims), dc.wgrad_steps(70))[0] == 4


@pytest.mark.parametrize("n", [5, 35])
@pytest.mark.parametrize("mode", ["sgld", "sgd", "swag", "bbb"])
@pytest.mark.parametrize("case,sizes_of", RUN_CASES, ids=[c.name for c, _ in RUN_CASES])
def test_resident_run_equals_single_steps(eng, case, sizes_of, mode, n):
    data = data_of(case)
    sizes = sizes_of(n)
    ragged = sizes[-1] != case.bmax
    call = call_of(case, mode, sizes)
    d = Dev(eng, case, mode, data, slots=48)
    start = rc.initial_state(mode, data, call.k)
    # the single steps; with a ragged last step also the state in front of it
    whole = call._replace(sizes=call.sizes[:-1], lrs=call.lrs[:-1]) if ragged else call
    d.reset(start)
    d.eager(whole)
    want = (d.state(), d.outputs())
    for use_graph in (True, False):
        d.reset(start)
        d.run(whole, use_graph=use_graph)
        assert (d.plan.last_run_path(), d.plan.last_run_graph_launches()) == rc.expected_run_path(len(whole.sizes), use_graph, True)
        got = (d.state(), d.outputs())
        assert_same(got, want, f"{case.name} {mode} {len(whole.sizes)} steps, graphs {use_graph}: run against single steps")
        assert written_slots(case, mode, got[1][0]) == list(range(case.slot0, case.slot0 + len(whole.sizes)))
        assert d.guards() == []
    if ragged:
        # the whole run, ragged last step included: graph against the eager-chained run bit for bit; against the single
        # steps the bound tests/test_gpu_run_matrix.py sets for its ragged chains (2e-6 of the largest magnitude)
        d.reset(start)
        d.eager(call)
        single = (d.state(), d.outputs())
        d.reset(start)
        d.run(call, use_graph=False)
        chained = (d.state(), d.outputs())
        d.reset(start)
        d.run(call, use_graph=True)
        assert d.plan.last_run_path() == ("graph", n)
        graph = (d.state(), d.outputs())
        assert_same(graph, chained, f"{case.name} {mode} {n} steps: graph against eager-chained run")
        lo, hi = case.slot0, case.slot0 + n - 1
        assert same_bits(chained[1][0][lo:hi], single[1][0][lo:hi]), f"{case.name} {mode}: the losses in front of the ragged step"
        assert written_slots(case, mode, graph[1][0]) == list(range(case.slot0, case.slot0 + n))
        for got, what in ((chained, "eager-chained run"), (graph, "graph run")):
            assert_same(got, single, f"{case.name} {mode} {n} steps, ragged last step: {what} against single steps", exact=False)
        assert d.guards() == []
    d.plan.check_finite()
    d.close()


@pytest.mark.parametrize("mode", ["sgld", "sgd", "swag", "bbb"])
@pytest.mark.parametrize("case,sizes_of", RUN_CASES, ids=[c.name for c, _ in RUN_CASES])
def test_launches_of_the_runs(eng, case, sizes_of, mode):
    data = data_of(case)
    d = Dev(eng, case, mode, data, slots=48)
    call = call_of(case, mode, sizes_of(5))
    d.reset(rc.initial_state(mode, data, call.k))
    got = probed(eng, d, call)
    want = rc.expected_run_launches(case, mode, 5)
    assert got == want, (case.name, mode, got[:12], want[:12])
    assert f"k_wgrad_all<{case.S}>" in got and got.count("k_bbb_sample") == (mode == "bbb")
    d.close()
