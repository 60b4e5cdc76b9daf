"""Host side of SGLD's lanes (pyz_sgld_lanes_step / pyz_sgld_lanes_run / pyz_lane_scores): the float64 restatement of one
P-lane step against oracle.philox and oracle.mlp directly, the comparison of tests/test_gpu_sgld_lanes.py rejecting the
wrong kernels on the CPU, the lane schedules against SGLD._init_sgld_lr, and the argument errors the library answers
without a GPU."""

import ctypes
import os
import re

import numpy as np
import pytest

import bce_checks
import sgld_lanes_checks as lc
from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.optimizers.SGLD import SGLD, lane_lr_table, resolve_lanes
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
from oracle import mlp as o_mlp
from oracle import philox as o_philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pyz_sgld_lanes_step": 16, "pyz_sgld_lanes_run": 17, "pyz_lane_scores": 9}


@pytest.fixture(autouse=True)
def bce(monkeypatch):
    bce_checks.install(monkeypatch)          # the oracle restated for the BCE case of the list


def test_lane_rates_are_all_different_and_none_below_the_case_rate():
    for case in lc.CASES:
        r = lc.lane_rates(case)
        assert r.shape == (case.P,) and len(set(r.tolist())) == case.P and r.min() == np.float32(case.step.lr)


# ---------------------------------------------------------------- the restatement against the oracle modules
@pytest.mark.parametrize("case", lc.CASES, ids=[c.name for c in lc.CASES])
def test_restatement_is_p_single_chain_steps_of_the_oracle(case):
    """Written out once more, directly: gradient from oracle.mlp at row c, z from oracle.philox with seed + c * stride, the
    three update lines with lr_c -- bit for bit what ref_lanes_step returns, in float64."""
    data = lc.chains_data(case)
    s0 = lc.initial_state(data)
    spec, st = case.step.spec, case.step
    rates = lc.lane_rates(case)
    for stride in lc.STRIDES:
        for variant in lc.VARIANTS:
            for k in (0, 2):
                ref = lc.ref_lanes_step(case, data, variant, k, s0, stride)
                n = np.float64(st.n0 + k)
                for c in range(case.P):
                    lr = np.float64(rates[c])
                    th0 = s0["theta"][c].astype(np.float64)
                    loss, g, _ = o_mlp.loss_and_grad(th0, data.step.rows, data.step.ys, spec, np.float64)
                    if variant == "zeros":
                        z = np.zeros(case.D)
                    else:
                        z = o_philox.normal(st.seed + c * stride, 0, st.n0 + k, case.D)
                        if variant == "philox":
                            z = z.astype(np.float32).astype(np.float64)
                    th = th0 + (-lr) * (g + lr * z)
                    assert np.array_equal(ref["theta"][c], th)
                    assert np.array_equal(ref["mean"][c], (s0["mean"][c].astype(np.float64) * n + th) / (n + 1.0))
                    assert np.array_equal(ref["sq"][c], (s0["sq"][c].astype(np.float64) * n + th ** 2) / (n + 1.0))
                    assert ref["loss"][c] == loss
                inj = lc.injected_noise(case, variant, k, stride)
                assert (inj is None) == (variant == "device")
                if variant == "philox":
                    for c in range(case.P):
                        assert np.array_equal(inj[c], o_philox.normal(st.seed + c * stride, 0, st.n0 + k, case.D).astype(np.float32))


# ---------------------------------------------------------------- the comparison sees the wrong kernels
@pytest.mark.parametrize("case", lc.CASES, ids=[c.name for c in lc.CASES])
def test_comparison_accepts_the_float32_step_and_rejects_every_mutation(case):
    data = lc.chains_data(case)
    s0 = lc.initial_state(data)
    for stride in lc.STRIDES:
        for variant in lc.VARIANTS:
            for k in range(lc.N_STEPS):
                ref = lc.ref_lanes_step(case, data, variant, k, s0, stride)
                lc.compare_lanes_step(case, k, s0, lc.as_stored(ref), ref, stride)     # the reference itself, as stored, passes
                for mutation in lc.MUTATIONS:
                    if not lc.mutation_applies(case, variant, stride, mutation):
                        continue
                    wrong = lc.as_stored(lc.ref_lanes_step(case, data, variant, k, s0, stride, mutation=mutation))
                    with pytest.raises(AssertionError):
                        lc.compare_lanes_step(case, k, s0, wrong, ref, stride, what=f"{mutation}: ")


def test_every_mutation_applies_somewhere():
    for mutation in lc.MUTATIONS:
        assert any(lc.mutation_applies(c, v, s, mutation) for c in lc.CASES for v in lc.VARIANTS for s in lc.STRIDES), mutation


# ---------------------------------------------------------------- the schedules
def test_lane_lr_table_columns_are_init_sgld_lr_of_each_lane():
    base = HyperParameters(lr_upper=0.02, lr_lower=0.005, lr_gamma=0.9, batch_size=16)
    lanes = resolve_lanes([{}, {"lr_upper": 0.05}, {"lr_gamma": 0.55, "lr_lower": 0.001},
                           HyperParameters(lr_upper=0.3, lr_lower=0.01, lr_gamma=0.7)], base)
    assert lanes[0] == {"lr_upper": 0.02, "lr_lower": 0.005, "lr_gamma": 0.9}
    assert lanes[1] == {"lr_upper": 0.05, "lr_lower": 0.005, "lr_gamma": 0.9}
    nb, n0, n_steps = 50, 7, 23
    table = lane_lr_table(lanes, nb, n0, n_steps)
    assert table.dtype == np.float32 and table.shape == (n_steps, 4) and table.flags["C_CONTIGUOUS"]
    for c, lane in enumerate(lanes):
        opt = SGLD()
        opt._lr_upper, opt._lr_lower, opt._lr_gamma, opt._nb_iterations = lane["lr_upper"], lane["lr_lower"], lane["lr_gamma"], nb
        opt._init_sgld_lr()
        # the way a quiet train() asks for its rates (one array) and the way step() does (one count)
        whole = np.asarray(opt._lr(n0 + np.arange(n_steps, dtype=np.float64))).astype(np.float32)
        single = np.array([np.float32(float(opt._lr(n0 + s))) for s in range(n_steps)], dtype=np.float32)
        assert np.array_equal(table[:, c].view(np.int32), whole.view(np.int32)), c
        assert np.array_equal(table[:, c].view(np.int32), single.view(np.int32)), c
        # a step's one-row table is the run's row
        for s in (0, 5, n_steps - 1):
            assert np.array_equal(lane_lr_table(lanes, nb, n0 + s, 1)[0].view(np.int32), table[s].view(np.int32))
    opt = SGLD()
    opt._lr_upper, opt._lr_lower, opt._lr_gamma, opt._nb_iterations = 0.02, 0.005, 0.9, nb
    opt._init_sgld_lr()
    assert float(opt._lr(0)) == pytest.approx(0.02, rel=1e-12) and float(opt._lr(nb)) == pytest.approx(0.005, rel=1e-12)


def test_resolve_lanes_refuses_other_keys_and_an_empty_list():
    base = HyperParameters(lr_upper=0.02, lr_lower=0.005, lr_gamma=0.9)
    with pytest.raises(ValueError, match="batch_size"):
        resolve_lanes([{"batch_size": 8}], base)
    with pytest.raises(ValueError, match="at least one lane"):
        resolve_lanes([], base)


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


def test_max_lanes_is_the_header_constant():
    src = open(os.path.join(ROOT, "include", "pyz.h")).read()
    assert int(re.search(r"#define\s+PYZ_MAX_LANES\s+(\d+)", src).group(1)) == _lib.MAX_LANES == 64


PARAMS = {
    "pyz_sgld_lanes_step": ("plan", "theta", "mean", "sq", "n_lanes", "x", "y", "row_idx", "batch", "lrs", "n", "seed", "stride",
                            "noise", "loss", "stream"),
    "pyz_sgld_lanes_run": ("plan", "theta", "mean", "sq", "n_lanes", "x", "y", "row_idx", "sizes", "lrs", "n_steps", "n", "slot0",
                           "seed", "stride", "loss", "stream"),
    "pyz_lane_scores": ("plan", "weights", "n_lanes", "x", "y", "rows", "loss", "errors", "stream"),
}


def call_args(name, **over):
    """Arguments that would be fine but for the plan (NULL: these calls must return before they look at it further):
    every pointer a dummy non-NULL address the library never follows, every number 1."""
    keep = []
    args = []
    for p, t in zip(PARAMS[name], _lib.SIGNATURES[name][1]):
        if p in over:
            v = over[p]
        elif p in ("plan", "stream", "noise", "errors"):
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


STEP_RUN_ERRORS = [
    ({}, b"null plan"),
    ({"n_lanes": 0}, b"n_lanes"),
    ({"n_lanes": -3}, b"n_lanes"),
    ({"n": -1}, b"negative step count"),
    ({"stride": 2}, b"seed_stride"),
    ({"stride": -1}, b"seed_stride"),
    ({"theta": None}, b"null"),
    ({"mean": None}, b"null"),
    ({"sq": None}, b"null"),
    ({"x": None}, b"null"),
    ({"y": None}, b"null"),
    ({"lrs": None}, b"null"),
    ({"loss": None}, b"null"),
]


@pytest.mark.parametrize("name", ["pyz_sgld_lanes_run", "pyz_sgld_lanes_step"])
@pytest.mark.parametrize("over,message", STEP_RUN_ERRORS)
def test_argument_errors_are_refused_without_a_gpu(name, over, message):
    lib = _lib.load()
    args, _keep = call_args(name, **over)
    assert getattr(lib, name)(*args) == -1                               # PYZ_E_INVALID
    err = lib.pyz_last_error()
    assert err and message in err, err


@pytest.mark.parametrize("over,message", [
    ({}, b"null plan"),
])
def test_lane_scores_refuses_a_null_plan_without_a_gpu(over, message):
    lib = _lib.load()
    args, _keep = call_args("pyz_lane_scores", **over)
    assert lib.pyz_lane_scores(*args) == -1
    err = lib.pyz_last_error()
    assert err and message in err, err
