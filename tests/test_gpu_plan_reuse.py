"""One plan across every entry point: the result of an op must not depend on what the plan did before it.

Every other GPU test file builds a fresh MLPPlan per case and drives one entry point on it; the arithmetic of each kernel
path is pinned to the float64 oracle there.  Here the plan is the object under test (tests/plan_reuse_cases.py lists its
state): the reference of an op is THE SAME OP ON A FRESH PLAN, computed once per (spec, op, call number), and every
comparison is bit for bit.

a. pairs     -- B after A on one plan == B's first call on a fresh plan, for every ordered pair of a spec's table.
b. triples   -- A, B, A for every graph-replaying A: the second A == the second call of A-then-A on a fresh plan; where B
                asks for more particles the plan's workspace must have grown across it (if a later change pre-sizes the
                buffers this fails and someone picks new shapes), and the capture counts say what ensure_bytes implies: a
                buffer that moved took every cached graph of the plan with it (recapture), nothing moved = replay.
c. stream    -- a graph captured on one side stream and replayed on another (the keys leave the stream out on purpose).
d. lazy ctl  -- an eager step leaves its StepCtl pending on the host; a read-out or lane_scores right behind it, then the
                step again.
e. sentinel  -- pyz_check_finite reports a non-finite loss once and resets (include/pyz.h); clean ops in between keep
                their bits and do not clear it.

At max_batch 8 an HMC proposal takes the one-workgroup form, which pyz_hmc_run launches eagerly: hmc_run is in the table
for its buffers and its feed / record state; hm_graphs and hmc_run_graphs get a plan of 192 rows of their own
(test_sliced_hmc_graphs_follow_a_moved_buffer)."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import plan_reuse_cases as pc  # noqa: E402

FULL_SPECS = ("narrow", "wide")
_BENCH = {}   # spec name -> (Env, ops): device tensors allocated once, addresses fixed for the whole module
_REF = {}     # (spec name, op name) -> [(arrays, info) of call 1, of call 2] on a fresh plan; never modified


@pytest.fixture(scope="module")
def eng(gpu_device):
    if "PYZ_GRAPH_STEPS" in os.environ:
        pytest.fail("PYZ_GRAPH_STEPS set in the environment: the expected graph counts assume its default -- unset it")
    from bayesian_inference_for_nn_amd import engine
    return engine


def bench(eng, spec_name):
    if spec_name not in _BENCH:
        env = pc.Env(pc.SPECS[spec_name], torch, eng)
        _BENCH[spec_name] = (env, pc.build_ops(env))
    return _BENCH[spec_name]


def info(plan, name):
    """What the info calls say about the last call of a run op (None for every other op)."""
    if name not in pc.GRAPH_CACHE:
        return None
    captures = getattr(plan, pc.CAPTURES_OF[pc.GRAPH_CACHE[name]])()
    return dict(path=plan.last_run_path(), launches=plan.last_run_graph_launches(), captures=captures)


def ref(eng, spec_name, name, call):
    """(arrays, info) of call 1 or 2 of A-then-A on a fresh plan."""
    if (spec_name, name) not in _REF:
        env, ops = bench(eng, spec_name)
        plan, a, calls = env.plan(), ops[name], []
        for _ in range(2):
            a.reset()
            out = a.call(plan)
            calls.append((out, info(plan, name)))
        plan.check_finite()
        plan.close()
        _REF[(spec_name, name)] = calls
    return _REF[(spec_name, name)][call - 1]


def spec_ops(specs=tuple(pc.SPECS)):
    return [(s, o) for s in specs for o in pc.op_names(s)]


def ids(pairs):
    return ["-".join(p) for p in pairs]


# ---------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("spec_name", list(pc.SPECS))
def test_a_then_a_replays_without_a_capture(eng, spec_name):
    """The info calls on a fresh plan: the first call captures, the same call again replays -- so no fix of the caches can be
    `always recapture` -- and both calls leave the same bits."""
    for name in pc.graph_ops(spec_name) + ("sgld_run_eager",):
        if name not in pc.TABLE[spec_name]:
            continue
        (r1, i1), (r2, i2) = ref(eng, spec_name, name, 1), ref(eng, spec_name, name, 2)
        assert pc.same_bits(r2, r1) == [], f"{spec_name} {name}: the second call on a fresh plan differs from the first"
        want = pc.first_call_info(name)
        assert i1 == want, (name, i1)
        assert i2 == dict(want, captures=0), (name, i2)


# ---------------------------------------------------------------- a. pairs
@pytest.mark.parametrize("spec_name,a", spec_ops(), ids=ids(spec_ops()))
def test_b_after_a_equals_b_on_a_fresh_plan(eng, spec_name, a):
    env, ops = bench(eng, spec_name)
    bad = []
    for b in ops:
        want = ref(eng, spec_name, b, 1)[0]
        plan = env.plan()
        ops[a].reset()
        ops[a].call(plan)
        ops[b].reset()
        out = ops[b].call(plan)
        diff = pc.same_bits(out, want)
        if diff:
            bad.append(f"{b} after {a}: {diff}")
        plan.check_finite()            # raises if any step of the two left a non-finite loss
        plan.close()
    assert not bad, f"{spec_name}: " + "; ".join(bad)


# ---------------------------------------------------------------- b. triples
def triple(eng, spec_name, a, b):
    """A, B, A on one plan: (arrays of the second A that differ from the reference, its info, workspace bytes before and after B)."""
    env, ops = bench(eng, spec_name)
    want = ref(eng, spec_name, a, 2)[0]
    plan = env.plan()
    ops[a].reset()
    ops[a].call(plan)
    ws0 = plan.workspace_bytes
    ops[b].reset()
    ops[b].call(plan)
    ws1 = plan.workspace_bytes
    ops[a].reset()
    out = ops[a].call(plan)
    got = info(plan, a)
    plan.check_finite()
    plan.close()
    return pc.same_bits(out, want), got, ws0, ws1


def graph_specs():
    return [(s, a) for s in pc.SPECS for a in pc.graph_ops(s)]


@pytest.mark.parametrize("spec_name,a", graph_specs(), ids=ids(graph_specs()))
def test_a_after_b_equals_a_after_a(eng, spec_name, a):
    _, ops = bench(eng, spec_name)
    want_info = ref(eng, spec_name, a, 2)[1]
    bad = []
    for b in ops:
        diff, got, ws0, ws1 = triple(eng, spec_name, a, b)
        if diff:
            bad.append(f"{a}, {b}, {a}: {diff}")
        if b in pc.GROWING_OPS and not ws1 > ws0:
            bad.append(f"{a}, {b}: the workspace did not grow across {b} ({ws0} -> {ws1} bytes): this pair no longer covers a moved buffer")
        # The other run of the same cache: a cache holds the graphs of ONE key (the caller's pointers and scalars), so B's run
        # replaced A's and A captures again.  Otherwise -- nothing allocated, nothing moved: a replay.  Something allocated: a
        # first allocation moves nothing (replay), a moved buffer drops every graph of the plan (the whole call is captured
        # again) -- never anything in between.
        n = pc.first_call_info(a)["captures"]
        if b != a and pc.GRAPH_CACHE.get(b) == pc.GRAPH_CACHE[a] and b != "sgld_run_eager":
            allowed = (n,)
        elif ws1 == ws0:
            allowed = (0,)
        elif (spec_name, a, b) in pc.MOVING_TRIPLES:
            allowed = (n,)
        else:
            allowed = (0, n)
        if got["captures"] not in allowed or dict(got, captures=0) != want_info:
            bad.append(f"{a}, {b}, {a}: info {got}, captures allowed {allowed} (workspace {ws0} -> {ws1})")
    assert not bad, f"{spec_name}: " + "; ".join(bad)


@pytest.mark.parametrize("spec_name,a,b", pc.MOVING_TRIPLES, ids=ids(pc.MOVING_TRIPLES))
def test_a_moved_buffer_drops_the_graphs(eng, spec_name, a, b):
    """B frees and reallocates a buffer that A's graphs (or A's eager launches) use: the second A must not replay through the
    old address.  Found by reading: on `wide` the chained SGLD step bakes m->grad into its launches and the key of m->graphs
    does not hold it."""
    diff, got, ws0, ws1 = triple(eng, spec_name, a, b)
    assert ws1 > ws0, f"the workspace did not grow across {b} ({ws0} -> {ws1}): pick shapes that move a buffer again"
    assert diff == [], f"{spec_name}: {a}, {b}, {a}: {diff}"
    assert got == pc.first_call_info(a)           # every cache of the plan was dropped: the call captures all its graphs again


def test_sliced_hmc_graphs_follow_a_moved_buffer(eng, monkeypatch):
    """hm_graphs and hmc_run_graphs, which the table's plans of 8 rows never fill: 192 rows put a proposal on the sliced form
    (k_hmc_multi: PYZ_HMC_RESIDENT=0 keeps the spin-waiting resident kernel out), pyz_hmc_step replays its one-proposal
    graph and pyz_hmc_run a graph of the four proposals behind its eager first one.  Behind a read-out both replay; behind
    a proposal of three chains, which moves hm_buf and the (P, D) buffers, the run captures again -- the same bits either way."""
    monkeypatch.setenv("PYZ_HMC_RESIDENT", "0")
    env = pc.Env(pc.SPECS["narrow"], torch, eng, n_rows=pc.SLICED_ROWS, max_batch=pc.SLICED_ROWS)
    ops = pc.build_ops(env, ("hmc_run_p1", "hmc_step_p1", "hmc_step_p3", "predict"))
    refs = {}
    for name, op in ops.items():
        plan, refs[name] = env.plan(), []
        for _ in range(2):
            op.reset()
            refs[name].append((op.call(plan), info(plan, name)))
        plan.check_finite()
        plan.close()
    assert refs["hmc_run_p1"][0][1] == dict(path=("mixed", pc.N_STEPS), launches=1, captures=1)
    assert refs["hmc_run_p1"][1][1] == dict(path=("mixed", pc.N_STEPS), launches=1, captures=0)
    for a in ("hmc_run_p1", "hmc_step_p1"):
        for b, moves in (("predict", False), ("hmc_step_p3", True)):
            plan = env.plan()
            ops[a].reset()
            ops[a].call(plan)
            ws0 = plan.workspace_bytes
            ops[b].reset()
            assert pc.same_bits(ops[b].call(plan), refs[b][0][0]) == [], f"{b} after {a}"
            assert (plan.workspace_bytes > ws0) == moves, f"{a}, {b}: workspace {ws0} -> {plan.workspace_bytes}"
            ops[a].reset()
            assert pc.same_bits(ops[a].call(plan), refs[a][1][0]) == [], f"{a}, {b}, {a}"
            if a == "hmc_run_p1":
                assert info(plan, a) == dict(path=("mixed", pc.N_STEPS), launches=1, captures=1 if moves else 0), f"{a}, {b}, {a}"
            plan.check_finite()
            plan.close()


# ---------------------------------------------------------------- c. stream
@pytest.mark.parametrize("a", ["sgld_run_graph", "adam_run"])
def test_a_graph_replays_on_another_stream(eng, a):
    env, ops = bench(eng, "narrow")
    want, want_info = ref(eng, "narrow", a, 2)
    plan = env.plan()
    ops[a].reset()
    ops[a].call(plan, stream=env.stream)
    ops[a].reset()
    out = ops[a].call(plan, stream=env.stream2)
    assert pc.same_bits(out, want) == []
    assert info(plan, a) == want_info            # (adam_run: captures == 0 -- the graph of the first stream was replayed)
    plan.check_finite()
    plan.close()


# ---------------------------------------------------------------- d. the pending StepCtl
LAZY = [(s, step, f) for s in FULL_SPECS for step in pc.EAGER_STEPS for f in pc.LAZY_CTL_FOLLOWERS]


@pytest.mark.parametrize("spec_name,step,follower", LAZY, ids=[f"pending ctl: {s} {a} then {b}" for s, a, b in LAZY])
def test_pending_ctl(eng, spec_name, step, follower):
    env, ops = bench(eng, spec_name)
    plan = env.plan()
    ops[step].reset()
    ops[step].call(plan)
    ops[follower].reset()
    assert pc.same_bits(ops[follower].call(plan), ref(eng, spec_name, follower, 1)[0]) == [], f"{follower} behind {step}"
    ops[step].reset()
    assert pc.same_bits(ops[step].call(plan), ref(eng, spec_name, step, 2)[0]) == [], f"{step} behind {follower}"
    plan.check_finite()
    plan.close()


# ---------------------------------------------------------------- e. the sentinel
@pytest.mark.parametrize("spec_name", FULL_SPECS)
def test_the_sentinel_reports_once_and_clean_ops_keep_their_bits(eng, spec_name):
    from bayesian_inference_for_nn_amd._lib import E_NAN, PyzError
    env, ops = bench(eng, spec_name)
    plan, step = env.plan(), ops["sgd_step"]

    def poisoned_step():
        step.reset()
        step.t["theta"][0] = float("nan")
        torch.cuda.synchronize()
        assert np.isnan(step.call(plan)["loss"]).all()

    def clean(names):
        for b in names:
            ops[b].reset()
            assert pc.same_bits(ops[b].call(plan), ref(eng, spec_name, b, 1)[0]) == [], f"{b} behind a non-finite step"

    # "returns PYZ_E_NAN if any step since the last call was non-finite ... and resets the count"
    poisoned_step()
    with pytest.raises(PyzError) as e:
        plan.check_finite()
    assert e.value.code == E_NAN
    plan.check_finite()                                       # reported once
    clean(("sgd_step", "sgld_run_graph", "predict", "hmc_step_p3"))
    plan.check_finite()
    # the count waits for its reader: clean ops behind the step neither clear it nor change
    poisoned_step()
    clean(("sgld_step", "sgld_run_graph", "lane_scores"))
    with pytest.raises(PyzError) as e:
        plan.check_finite()
    assert e.value.code == E_NAN
    plan.check_finite()
    plan.close()
