"""Host side of SGLD's n_chains (pyz_sgld_chains_step / pyz_sgld_chains_run): the float64 restatement of one P-chain step
against oracle.philox and oracle.mlp directly, the comparison of tests/test_gpu_sgld_chains.py rejecting the wrong kernels
on the CPU, the case list reaching what it has to, the pooling rule and R-hat against closed forms, and the argument errors
the library answers without a GPU."""

import ctypes
import os
import re

import numpy as np
import pytest

import bce_checks
import sgld_chains_checks as cc
import step_cases as sc
from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.optimizers.SGLD import gelman_rubin, pool_chain_moments
from oracle import mlp as o_mlp
from oracle import philox as o_philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pyz_sgld_chains_step": 15, "pyz_sgld_chains_run": 17}


@pytest.fixture(autouse=True)
def bce(monkeypatch):
    bce_checks.install(monkeypatch)          # the oracle restated for the BCE case of the list


# ---------------------------------------------------------------- the case list
def test_cases_reach_every_way_the_kernel_can_go_wrong():
    cov = cc.coverage()
    assert cov["P"] >= {1, 2, 5}
    assert cov["D % 4"] == {0, 1, 2, 3}
    assert cov["aligned"] == {True, False} and cov["fused"] == {True, False}
    assert cov["loss"] == {"scce", "mse", "bce"}
    for key in ("more than one workgroup per chain", "odd batch", "gathered with a ragged N", "last layer of 33",
                "unaligned rows behind an aligned first row"):
        assert cov[key], key
    for case in cc.CASES:
        assert case.step.n0 == 3 and max(case.step.dims) <= 40 and 5 <= case.step.batch <= 37, case.name
        assert case.D == case.step.D


# ---------------------------------------------------------------- the restatement against the oracle modules
@pytest.mark.parametrize("case", cc.CASES, ids=[c.name for c in cc.CASES])
def test_restatement_is_p_single_chain_steps_of_the_oracle(case):
    """Written out once more, directly: gradient from oracle.mlp at row c, z from oracle.philox with seed + c, the three
    update lines -- bit for bit what ref_chains_step returns, in float64."""
    data = cc.chains_data(case)
    s0 = cc.initial_state(data)
    assert len({data.theta0[c].tobytes() for c in range(case.P)}) == case.P       # every chain has a start of its own
    spec, st = case.step.spec, case.step
    for variant in cc.VARIANTS:
        for k in (0, 2):
            ref = cc.ref_chains_step(case, data, variant, k, s0)
            n, lr = np.float64(st.n0 + k), np.float64(st.lr)
            for c in range(case.P):
                th0 = s0["theta"][c].astype(np.float64)
                loss, g, _ = o_mlp.loss_and_grad(th0, data.step.rows, data.step.ys, spec, np.float64)
                if variant == "zeros":
                    z = np.zeros(case.D)
                else:
                    z = o_philox.normal(st.seed + c, 0, st.n0 + k, case.D)
                    if variant == "philox":
                        z = z.astype(np.float32).astype(np.float64)
                th = th0 + (-lr) * (g + lr * z)
                assert np.array_equal(ref["theta"][c], th)
                assert np.array_equal(ref["mean"][c], (s0["mean"][c].astype(np.float64) * n + th) / (n + 1.0))
                assert np.array_equal(ref["sq"][c], (s0["sq"][c].astype(np.float64) * n + th ** 2) / (n + 1.0))
                assert ref["loss"][c] == loss
            inj = cc.injected_noise(case, variant, k)
            assert (inj is None) == (variant == "device")
            if variant == "philox":
                for c in range(case.P):
                    assert np.array_equal(inj[c], o_philox.normal(st.seed + c, 0, st.n0 + k, case.D).astype(np.float32))


# ---------------------------------------------------------------- the comparison sees the wrong kernels
@pytest.mark.parametrize("case", cc.CASES, ids=[c.name for c in cc.CASES])
def test_comparison_accepts_the_float32_step_and_rejects_every_mutation(case):
    data = cc.chains_data(case)
    s0 = cc.initial_state(data)
    for variant in cc.VARIANTS:
        for k in range(cc.N_STEPS):
            ref = cc.ref_chains_step(case, data, variant, k, s0)
            cc.compare_chains_step(case, k, s0, cc.as_stored(ref), ref)           # the reference itself, as stored, passes
            for mutation in cc.MUTATIONS:
                if not cc.mutation_applies(case, variant, mutation):
                    continue
                wrong = cc.as_stored(cc.ref_chains_step(case, data, variant, k, s0, mutation=mutation))
                with pytest.raises(AssertionError):
                    cc.compare_chains_step(case, k, s0, wrong, ref, what=f"{mutation}: ")


def test_every_mutation_applies_somewhere():
    for mutation in cc.MUTATIONS:
        assert any(cc.mutation_applies(c, v, mutation) for c in cc.CASES for v in cc.VARIANTS), mutation


# ---------------------------------------------------------------- pooling and R-hat
def test_pooling_is_the_count_weighted_average_over_chains():
    P, D = 4, 7
    mean = np.full((P, D), 2.0, dtype=np.float32)
    mean[0] = 0.0
    sq = mean.copy()
    m, s = pool_chain_moments(mean, sq)
    assert m.dtype == np.float64 and np.array_equal(m, np.full(D, 1.5)) and np.array_equal(s, np.full(D, 1.5))
    # merge_moment_chains' rule with equal counts: sum_c n m_c / sum_c n
    n = 13.0
    assert np.array_equal(m, (n * mean.astype(np.float64)).sum(axis=0) / (n * P))
    # float64 accumulation: float32 would lose the small chain beside the large ones
    big = np.array([[16777216.0], [1.0], [1.0]], dtype=np.float32)
    assert pool_chain_moments(big, big)[0][0] == (16777216.0 + 2.0) / 3.0


def test_r_hat_of_identical_chains():
    rng = np.random.default_rng(0)
    D, n = 9, 17
    m = rng.normal(size=D)
    sq = m ** 2 + rng.uniform(0.1, 1.0, size=D)
    got = gelman_rubin(np.stack([m, m, m]), np.stack([sq, sq, sq]), n)
    assert got.dtype == np.float64 and got.shape == (D,)
    np.testing.assert_allclose(got, np.sqrt((n - 1) / n), rtol=1e-12)


def test_r_hat_of_a_hand_computed_two_chain_case():
    """One parameter, n = 5 draws: chain A = 0, 1, 2, 3, 4 (mean 2, mean of squares 6, sample variance 2.5), chain B =
    4, 5, 6, 7, 8 (mean 6, mean of squares 38, sample variance 2.5).  W = 2.5, B / n = var(2, 6; ddof 1) = 8,
    R-hat = sqrt((0.8 * 2.5 + 8) / 2.5) = 2."""
    a, b = np.arange(5.0), np.arange(4.0, 9.0)
    mean = np.array([[a.mean()], [b.mean()]])
    sq = np.array([[(a ** 2).mean()], [(b ** 2).mean()]])
    assert mean.tolist() == [[2.0], [6.0]] and sq.tolist() == [[6.0], [38.0]]
    assert gelman_rubin(mean, sq, 5)[0] == pytest.approx(2.0, rel=1e-14)


def test_r_hat_refuses_one_chain_and_one_step():
    m = np.zeros((1, 3))
    with pytest.raises(ValueError):
        gelman_rubin(m, m, 10)
    m = np.zeros((2, 3))
    with pytest.raises(ValueError):
        gelman_rubin(m, m, 1)


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


def call_args(name, **over):
    """Arguments that would be fine but for the plan (NULL: these calls must return before they look at it further):
    every pointer a dummy non-NULL address the library never follows, every number 1."""
    params = {"pyz_sgld_chains_step": ("plan", "theta", "mean", "sq", "n_chains", "x", "y", "row_idx", "batch", "lr", "n",
                                       "seed", "noise", "loss", "stream"),
              "pyz_sgld_chains_run": ("plan", "theta", "mean", "sq", "n_chains", "x", "y", "row_idx", "sizes", "lrs",
                                      "n_steps", "n", "slot0", "seed", "loss", "use_graph", "stream")}[name]
    keep = []
    args = []
    for p, t in zip(params, _lib.SIGNATURES[name][1]):
        if p in over:
            v = over[p]
        elif p in ("plan", "stream", "noise"):
            v = None
        elif t is ctypes.c_void_p:
            v = ctypes.c_void_p(4096)
        elif t is ctypes.POINTER(ctypes.c_int32):
            keep.append((ctypes.c_int32 * 1)(1))
            v = keep[-1]
        elif t is ctypes.POINTER(ctypes.c_float):
            keep.append((ctypes.c_float * 1)(0.5))
            v = keep[-1]
        elif t is ctypes.c_float:
            v = 0.5
        else:
            v = 1
        args.append(v)
    return args, keep


@pytest.mark.parametrize("name", sorted(NAMES))
@pytest.mark.parametrize("over,message", [
    ({}, b"null plan"),
    ({"n_chains": 0}, b"n_chains"),
    ({"n": -1}, b"negative step count"),
    ({"theta": None}, b"null"),
    ({"mean": None}, b"null"),
    ({"sq": None}, b"null"),
    ({"x": None}, b"null"),
    ({"y": None}, b"null"),
    ({"loss": None}, b"null"),
])
def test_argument_errors_are_refused_without_a_gpu(name, over, message):
    lib = _lib.load()
    args, _keep = call_args(name, **over)
    assert getattr(lib, name)(*args) == -1                               # PYZ_E_INVALID
    err = lib.pyz_last_error()
    assert err and message in err, err
