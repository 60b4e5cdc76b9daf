"""Host side of BBB's lanes (pyz_bbb_lanes_step / pyz_bbb_lanes_run, BBB.compile's lanes, BBBGridObjective): a float32
stand-in of the restatement under the comparison of tests/test_gpu_bbb_lanes.py, that comparison rejecting the wrong kernels
on the CPU, the refusals of resolve / compile before any device work, the grid objective's grouping with a stubbed trainer,
and the argument errors the library answers without a GPU."""

import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import bbb_lanes_checks as bl
import bce_checks
from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.distributions import GaussianPrior
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import BBBGridObjective, GridOptimizer, HyperParameters, Real
from bayesian_inference_for_nn_amd.optimizers.hyperparameters.GridOptimizer import LanesGridObjective, SGLDGridObjective

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pyz_bbb_lanes_step": 21, "pyz_bbb_lanes_run": 22}
bbb_module = importlib.import_module("bayesian_inference_for_nn_amd.optimizers.BBB")


@pytest.fixture(autouse=True)
def bce(monkeypatch):
    bce_checks.install(monkeypatch)          # the oracle restated for the BCE case of the list


def test_the_cases_are_the_nine_chain_shapes_with_the_lane_numbers_of_the_issue():
    assert [c.name for c in bl.CASES] == [c.name for c in bl.cc.CASES]
    assert sum(c.step.prior_vec for c in bl.CASES) == 2
    zero = 0
    for case in bl.CASES:
        t = bl.lane_tables(case)
        st = case.step
        for c in range(case.P):
            lane = bl.lane_case(case, c, 1)
            assert lane.bbb_lr == st.bbb_lr * (1 + c / 4) and lane.prior == (st.prior[0] + c / 8, st.prior[1] - c / 4)
            assert lane.seed == st.seed + c and bl.lane_case(case, c, 0).seed == st.seed
        assert len(set(t.alpha.tolist())) == case.P and len(set(t.lr.tolist())) == case.P
        zero += int((t.alpha == 0).sum())
    assert zero == 1                                                       # one lane of one case at alpha = 0


# ---------------------------------------------------------------- the comparison: a float32 stand-in passes, wrong kernels do not
@pytest.mark.parametrize("case", bl.CASES, ids=[c.name for c in bl.CASES])
def test_comparison_accepts_a_float32_step_and_rejects_every_mutation(case):
    data = bl.lanes_data(case)
    s0 = bl.initial_state(data)
    rejected = set()
    for stride in bl.STRIDES:
        for variant in bl.VARIANTS:
            ref = bl.ref_bbb_lanes_step(case, data, variant, 0, s0, stride)
            stand_in = bl.as_stored(bl.ref_bbb_lanes_step(case, data, variant, 0, s0, stride, dtype=np.float32))
            bl.compare_bbb_lanes_step(case, 0, s0, stand_in, ref, stride, what=f"float32 stride {stride} {variant}: ")
            bl.compare_bbb_lanes_step(case, 0, s0, bl.as_stored(ref), ref, stride)
            for mutation in bl.MUTATIONS:
                if not bl.mutation_applies(case, variant, stride, mutation):
                    continue
                wrong = bl.as_stored(bl.ref_bbb_lanes_step(case, data, variant, 0, s0, stride, mutation=mutation))
                with pytest.raises(AssertionError):
                    bl.compare_bbb_lanes_step(case, 0, s0, wrong, ref, stride, what=f"{mutation}: ")
                rejected.add(mutation)
    assert (len(rejected) >= 1) == (case.P >= 2)


def test_float32_stand_in_passes_every_step_from_the_start_and_the_walk_where_the_reference_stays_put():
    """The steps as the GPU test takes them.  From the start: every case, Philox steps n0 .. n0 + 2.  One after the other
    (the reference restarts from the state the stand-in stored): the cases of WALK, which are exactly those whose float64
    reference keeps every lane's rho at or above WALK_RHO_MIN."""
    for case in bl.CASES:
        data = bl.lanes_data(case)
        start = bl.initial_state(data)
        for k in range(bl.N_STEPS):
            ref = bl.ref_bbb_lanes_step(case, data, "philox", k, start, 1)
            got = bl.as_stored(bl.ref_bbb_lanes_step(case, data, "philox", k, start, 1, dtype=np.float32))
            bl.compare_bbb_lanes_step(case, k, start, got, ref, 1, what=f"float32 step {k} from the start: ")
        s0, lo = start, np.inf
        for k in range(bl.N_STEPS):
            ref = bl.ref_bbb_lanes_step(case, data, "philox", k, s0, 1)
            lo = min(lo, ref["rho"].min())
            if case.name in bl.WALK:
                got = bl.as_stored(bl.ref_bbb_lanes_step(case, data, "philox", k, s0, 1, dtype=np.float32))
                bl.compare_bbb_lanes_step(case, k, s0, got, ref, 1, what=f"float32 step {k} of the walk: ")
            s0 = {key: np.asarray(ref[key], dtype=np.float32) for key in ("mu", "rho", "w")}
        assert (bl.WALK_RHO_MIN <= lo) == (case.name in bl.WALK), (case.name, lo)


def test_every_mutation_applies_somewhere():
    for mutation in bl.MUTATIONS:
        assert any(bl.mutation_applies(c, v, s, mutation) for c in bl.CASES for v in bl.VARIANTS for s in bl.STRIDES), mutation


# ---------------------------------------------------------------- resolve / compile refusals, before any device work
def test_resolve_lanes_fills_in_the_base_and_refuses_what_does_not_differ_between_lanes():
    base = HyperParameters(lr=0.01, alpha=0.5, batch_size=16)
    lanes = bbb_module.resolve_lanes([{}, {"lr": 0.1}, {"pi": 0.25, "alpha": 0.0}, HyperParameters(lr=0.3, alpha=0.2)], base)
    assert lanes == [{"lr": 0.01, "alpha": 0.5, "pi": 1}, {"lr": 0.1, "alpha": 0.5, "pi": 1},
                     {"lr": 0.01, "alpha": 0.0, "pi": 0.25}, {"lr": 0.3, "alpha": 0.2, "pi": 1}]
    assert bbb_module.resolve_lanes([{}], HyperParameters(lr=0.01, alpha=0.5, pi=0.75))[0]["pi"] == 0.75
    assert bbb_module.LANE_KEYS == ("lr", "alpha", "pi")
    with pytest.raises(ValueError, match="batch_size"):
        bbb_module.resolve_lanes([{"batch_size": 8}], base)
    with pytest.raises(ValueError, match="momentum"):
        bbb_module.resolve_lanes([{"momentum": 0.9}], base)
    with pytest.raises(ValueError, match="at least one lane"):
        bbb_module.resolve_lanes([], base)
    listed = GaussianPrior([0.0, 0.0], [1.0, 1.0])
    with pytest.raises(ValueError, match="list-valued"):
        bbb_module.resolve_lanes([{"pi": 0.5}], base, listed)
    assert bbb_module.resolve_lanes([{"lr": 0.5}], base, listed)[0]["pi"] == 1


def test_mix_prior_is_the_formula_of_compile():
    p = bbb_module.mix_prior(GaussianPrior(0.5, -2.0), GaussianPrior(0.25, 1.0), 0.25)
    assert p._mean == 0.5 * 0.25 + 0.25 * 0.75
    assert p._std_dev == -np.sqrt((2.0 * 0.25) ** 2 + (1.0 * 0.75) ** 2)


def test_compile_refuses_before_it_builds_a_plan(monkeypatch):
    from bayesian_inference_for_nn_amd import parallel
    from bayesian_inference_for_nn_amd.nn import sequential_json
    from bayesian_inference_for_nn_amd.optimizers.Optimizer import Optimizer

    def no_device(*a, **kw):
        raise AssertionError("the backend was set up")
    monkeypatch.setattr(Optimizer, "_setup_backend", no_device)
    hp = HyperParameters(lr=0.01, alpha=0.5, batch_size=16)
    cfg = sequential_json(2, [4, 2], ["relu", "softmax"])
    prior = GaussianPrior(0.0, -2.0)

    def compile_with(**kw):
        bbb_module.BBB().compile(hp, cfg, None, verbose=False, prior=kw.pop("prior", prior), **kw)
    for kw in ({"lanes": []}, {"lanes": [{"lr_upper": 0.1}]}, {"lanes": [{}], "lane_seeds": "random"},
               {"lanes": [{"pi": 0.5}], "prior": GaussianPrior([0.0, 0.0], [1.0, 1.0])}):
        with pytest.raises(ValueError):
            compile_with(**kw)
    monkeypatch.setattr(parallel, "world_info", lambda: (0, 2))
    with pytest.raises(ValueError, match="one rank"):
        compile_with(lanes=[{}])
    monkeypatch.setattr(parallel, "world_info", lambda: (0, 1))
    with pytest.raises(AssertionError, match="backend"):                   # a good list does go on to the backend
        compile_with(lanes=[{}, {"lr": 0.1}])


# ---------------------------------------------------------------- the grid objective with a stubbed trainer
def test_grid_objective_groups_by_batch_size_and_chunks_by_max_lanes(monkeypatch):
    hp = HyperParameters(lr=0.01, alpha=0.5, batch_size=16)
    seen = []

    def trainer(self, batch_size, lanes):
        seen.append((batch_size, [dict(l) for l in lanes]))
        return self._values(len(lanes), {"loss": None, "error": [l["lr"] * 10 + l["alpha"] for l in lanes]})
    monkeypatch.setattr(BBBGridObjective, "_train_chunk", trainer)
    obj = BBBGridObjective(hp, "{}", None, 10, GaussianPrior(0.0, -2.0), max_lanes=4)
    grid = GridOptimizer()
    grid.compile(obj, Real(0.1, 0.3, "lr"), Real(0.0, 1.0, "alpha"), n=3, specify={"alpha": [0.25, 0.75]}, verbose=False)
    grid.optimize()
    points = list(grid.results)
    assert len(points) == 6 and obj.trainings == [4, 2]
    assert [len(lanes) for _, lanes in seen] == [4, 2] and {b for b, _ in seen} == {16}
    assert [grid.results[p] for p in points] == [p[0] * 10 + p[1] for p in points]           # values in point order
    assert grid.best()[1] == min(grid.results.values())
    # batch sizes make groups of their own; a score that is not finite becomes inf; one point through __call__
    seen.clear()
    monkeypatch.setattr(BBBGridObjective, "_train_chunk",
                        lambda self, b, lanes: self._values(len(lanes), {"error": [float("nan") if b == 8 else 1.0] * len(lanes)}))
    out = obj.evaluate_lanes(["lr", "batch_size"], [(0.1, 16), (0.2, 8), (0.3, 16)])
    assert out == [1.0, float("inf"), 1.0] and obj.trainings == [4, 2, 2, 1]
    assert obj(0.1, 0.5, 0.25) == 1.0 and obj.trainings[-1] == 1
    with pytest.raises(ValueError, match="lr_upper"):
        obj.evaluate_lanes(["lr_upper"], [(0.1,)])
    assert BBBGridObjective.NAMES == ("lr", "alpha", "pi", "batch_size")
    for bad in ({"metric": "accuracy"}, {"weights": "theta"}, {"max_lanes": 0}, {"nb_samples": 0},
                {"weights": "predictive", "metric": "val_loss"}):
        with pytest.raises(ValueError):
            BBBGridObjective(hp, "{}", None, 10, GaussianPrior(0.0, -2.0), **bad)


def test_both_objectives_share_one_grouping():
    for cls in (SGLDGridObjective, BBBGridObjective):
        assert issubclass(cls, LanesGridObjective)
        assert "evaluate_lanes" not in vars(cls) and "__call__" not in vars(cls)


# ---------------------------------------------------------------- the C boundary without a GPU
def header_arity(name):
    src = open(os.path.join(ROOT, "include", "pyz.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/pyz.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_in_header_and_ctypes_table_with_matching_arity(name):
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int
    assert len(argtypes) == header_arity(name) == NAMES[name]
    assert _lib.header_version() == 302                                  # the new entry points do not move the version
    assert _lib.load().pyz_version() == 302


PARAMS = {
    "pyz_bbb_lanes_step": ("plan", "mu", "rho", "w", "n_lanes", "x", "y", "row_idx", "batch", "lr", "alpha", "pm", "pr", "pm_vec",
                           "pr_vec", "step", "seed", "stride", "eps", "cost", "stream"),
    "pyz_bbb_lanes_run": ("plan", "mu", "rho", "w", "n_lanes", "x", "y", "lr", "alpha", "pm", "pr", "pm_vec", "pr_vec", "row_idx",
                          "sizes", "n_steps", "step", "slot0", "seed", "stride", "cost", "stream"),
}


def call_args(name, **over):
    """Arguments that would be fine but for the plan (NULL: these calls must return before they look at it further): every
    pointer a dummy non-NULL address the library never follows, every number 1."""
    keep, args = [], []
    for p, t in zip(PARAMS[name], _lib.SIGNATURES[name][1]):
        if p in over:
            v = over[p]
        elif p in ("plan", "stream", "eps", "pm_vec", "pr_vec"):
            v = None
        elif t is ctypes.c_void_p:
            v = ctypes.c_void_p(4096)
        elif t is ctypes.POINTER(ctypes.c_int32):
            keep.append((ctypes.c_int32 * 1)(1))
            v = keep[-1]
        elif t is ctypes.POINTER(ctypes.c_float):
            keep.append((ctypes.c_float * 1)(0.5))
            v = keep[-1]
        else:
            v = 1
        args.append(v)
    return args, keep


INVALID = [
    ({}, b"null plan"),
    ({"n_lanes": 0}, b"n_lanes"),
    ({"n_lanes": -3}, b"n_lanes"),
    ({"step": -1}, b"negative step"),
    ({"stride": 2}, b"seed_stride"),
    ({"stride": -1}, b"seed_stride"),
    ({"pm_vec": ctypes.c_void_p(4096)}, b"prior vectors"),
    ({"pr_vec": ctypes.c_void_p(4096)}, b"prior vectors"),
] + [({p: None}, b"null") for p in ("mu", "rho", "w", "x", "y", "lr", "alpha", "pm", "pr", "cost")]


@pytest.mark.parametrize("name", sorted(NAMES))
@pytest.mark.parametrize("over,message", INVALID, ids=[",".join(f"{k}={getattr(v, 'value', v)}" for k, v in o.items()) or "plan"
                                                        for o, _ in INVALID])
def test_argument_errors_are_refused_without_a_gpu(name, over, message):
    lib = _lib.load()
    args, _keep = call_args(name, **over)
    assert getattr(lib, name)(*args) == -1                               # PYZ_E_INVALID
    err = lib.pyz_last_error()
    assert err and message in err, err


@pytest.mark.parametrize("name", sorted(NAMES))
def test_more_lanes_than_the_library_takes_is_a_shape_error_without_a_gpu(name):
    lib = _lib.load()
    args, _keep = call_args(name, n_lanes=_lib.MAX_LANES + 1)
    assert getattr(lib, name)(*args) == -2                               # PYZ_E_SHAPE, before the plan is looked at
    assert b"n_lanes" in lib.pyz_last_error()
    args, _keep = call_args(name, n_lanes=_lib.MAX_LANES)
    assert getattr(lib, name)(*args) == -1 and b"null plan" in lib.pyz_last_error()


def test_run_refuses_its_own_null_tables_without_a_gpu():
    lib = _lib.load()
    for p in ("row_idx", "sizes"):
        args, _keep = call_args("pyz_bbb_lanes_run", **{p: None})
        assert lib.pyz_bbb_lanes_run(*args) == -1
