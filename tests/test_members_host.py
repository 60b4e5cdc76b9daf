"""Host side of SGD / SWAG n_members (pyz_sgd_members_step / _run, pyz_swag_members_step / _run) and of the Mixture
distribution: the comparison of tests/test_gpu_members.py rejecting the wrong kernels on the CPU, the case list reaching
what it has to, the run's hit / column rule against oracle.swag, the C boundary without a GPU, Mixture's draws and its
store / load, and the starting_model list."""

import ctypes
import os
import random
import re

import numpy as np
import pytest

import bce_checks
import members_checks as mc
import step_cases as sc
from bayesian_inference_for_nn_amd import _lib
from oracle import mlp as o_mlp
from oracle import swag as o_swag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pyz_sgd_members_step": 13, "pyz_sgd_members_run": 16, "pyz_swag_members_step": 17, "pyz_swag_members_run": 19}


@pytest.fixture(autouse=True)
def bce(monkeypatch):
    bce_checks.install(monkeypatch)          # the oracle restated for the BCE case of the list


# ---------------------------------------------------------------- the case list
def test_cases_reach_every_way_the_kernel_can_go_wrong():
    cov = mc.coverage()
    assert cov["P"] >= {1, 2, 5}
    assert cov["D % 4"] == {0, 1, 2, 3}
    assert cov["aligned"] == {True, False} and cov["fused"] == {True, False}
    assert cov["loss"] == {"scce", "mse", "bce"}
    assert cov["modes"] == {"sgd", "swag"}
    assert cov["SWAG steps"] == {(True, 1), (False, 0), (True, None)} and cov["SGD hits"] == {True, False}
    for key in ("more than one workgroup per member", "odd batch", "gathered with a ragged N", "last layer of 33",
                "unaligned rows behind an aligned first row", "deviation rows of both alignments in one launch"):
        assert cov[key], key
    assert mc.SWAG_STEPS is sc.SWAG_STEPS and mc.SGD_HITS == (True, False, True) and mc.K_DEV == 2
    assert any(c.D == 1100 and c.P > 1 for c in mc.CASES)


# ---------------------------------------------------------------- the comparison sees the wrong kernels
@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("case", mc.CASES, ids=[c.name for c in mc.CASES])
def test_comparison_accepts_the_float32_step_and_rejects_every_mutation(case, mode):
    data = mc.members_data(case)
    s0 = mc.initial_state(case, mode, data)
    assert len({data.theta0[c].tobytes() for c in range(case.P)}) == case.P        # every member has a start of its own
    for k in range(mc.N_STEPS):
        ref = mc.ref_members_step(case, data, mode, k, s0)
        if mode == "sgd":      # (SWAG's deviation row is float32(theta) - float32(mean) exactly: only float32 arithmetic gives it)
            mc.compare_members_step(case, mode, k, s0, mc.as_stored(ref), ref)      # the reference itself, as stored
        f32 = mc.ref_members_step(case, data, mode, k, s0, dtype=np.float32)        # the float32 restatement
        assert all(np.asarray(v).dtype == np.float32 for v in f32.values())
        mc.compare_members_step(case, mode, k, s0, f32, ref, what="float32: ")
        for mutation in mc.MUTATIONS:
            if not mc.mutation_applies(case, mode, k, mutation):
                continue
            wrong = mc.ref_members_step(case, data, mode, k, s0, dtype=np.float32, mutation=mutation)
            with pytest.raises(AssertionError):
                mc.compare_members_step(case, mode, k, s0, wrong, ref, what=f"{mutation}: ")


def test_every_mutation_applies_somewhere():
    for mutation in mc.MUTATIONS:
        assert any(mc.mutation_applies(c, m, k, mutation) for c in mc.CASES for m in mc.MODES for k in range(mc.N_STEPS)), mutation


def test_restatement_is_p_single_model_steps():
    """Row c of the P-member reference is step_cases.ref_step of row c, bit for bit; SGD's mean is the new weights after
    a hit and the old mean after a miss."""
    case = mc.CASE_BY_NAME["f_d66_gathered_p5"]
    data = mc.members_data(case)
    for mode in mc.MODES:
        s0 = mc.initial_state(case, mode, data)
        for k in range(mc.N_STEPS):
            ref = mc.ref_members_step(case, data, mode, k, s0)
            for c in range(case.P):
                one = sc.ref_step(case.step, data.step, mode, "plain", k, mc.member_state(s0, c))
                for key, v in one.items():
                    assert np.array_equal(np.asarray(ref[key][c]), np.asarray(v)), (mode, k, c, key)
                if mode == "sgd":
                    want = one["theta"] if mc.SGD_HITS[k] else s0["mean"][c].astype(np.float64)
                    assert np.array_equal(ref["mean"][c], want)


# ---------------------------------------------------------------- the run's rules
@pytest.mark.parametrize("freq,k", [(1, 2), (3, 3), (4, 1)])
def test_run_hit_and_column_rule_is_append_then_replace_last(freq, k):
    """oracle.swag.swag_step over 14 counts: a step is a hit when its deviation matrix changes, and the row it writes is
    the appended one until there are k, then the last."""
    spec = o_mlp.MLPSpec((1, 1), ("linear",), "mse")
    x, y = np.array([[0.5], [-1.0]]), np.array([[1.0], [0.25]])
    st = o_swag.SWAGState(np.array([0.3, -0.2]), k)
    hits = 0
    for n in range(14):
        before = st.dev.copy()
        assert st.n == n
        o_swag.swag_step(st, x, y, spec, 0.1, freq)
        hit = st.dev.shape != before.shape or not np.array_equal(st.dev, before)
        assert hit == mc.run_hit(n, freq), (n, freq)
        if hit:
            written = before.shape[0] if before.shape[0] < k else k - 1
            assert np.array_equal(st.dev[written], st.theta - st.mean)
            assert written == mc.run_column(n, freq, k), (n, freq, k)
            hits += 1
        assert st.dev.shape[0] == min(hits, k)
    assert hits == -(-14 // freq)


# ---------------------------------------------------------------- the C boundary without a GPU
def header_arity(name):
    src = open(os.path.join(ROOT, "include", "pyz.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/pyz.h"
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


def ctype_of(decl):
    if "*" in decl:
        if decl.startswith("const int32_t *h_"):
            return ctypes.POINTER(ctypes.c_int32)
        if decl.startswith("const float *h_"):
            return ctypes.POINTER(ctypes.c_float)
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}[decl.split()[0]]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_in_header_with_argtypes_matching_the_ctypes_table(name):
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int
    decls = header_arity(name)
    assert len(argtypes) == len(decls) == NAMES[name]
    assert [ctype_of(d) for d in decls] == list(argtypes), decls
    assert _lib.header_version() == 302                                  # the new entry points do not move the version


PARAMS = {
    "pyz_sgd_members_step": ("plan", "theta", "mean", "n_members", "x", "y", "row_idx", "batch", "lr", "n", "update", "loss",
                             "stream"),
    "pyz_sgd_members_run": ("plan", "theta", "mean", "n_members", "frequency", "x", "y", "row_idx", "sizes", "lrs", "n_steps",
                            "n", "slot0", "loss", "use_graph", "stream"),
    "pyz_swag_members_step": ("plan", "theta", "mean", "sq", "dev", "k", "n_members", "x", "y", "row_idx", "batch", "lr", "n",
                              "update", "col", "loss", "stream"),
    "pyz_swag_members_run": ("plan", "theta", "mean", "sq", "dev", "k", "frequency", "n_members", "x", "y", "row_idx", "sizes",
                             "lrs", "n_steps", "n", "slot0", "loss", "use_graph", "stream"),
}


def call_args(name, **over):
    """Arguments that would be fine but for the plan (NULL: these calls must return before they look at it further):
    every pointer a dummy non-NULL address the library never follows, every number 1 (the column 0)."""
    keep, args = [], []
    for p, t in zip(PARAMS[name], _lib.SIGNATURES[name][1]):
        if p in over:
            v = over[p]
        elif p in ("plan", "stream"):
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
            v = 0 if p == "col" else 1
        args.append(v)
    return args, keep


ERRORS = [({}, b"null plan"), ({"n_members": 0}, b"n_members"), ({"n": -1}, b"negative step count"), ({"theta": None}, b"null"),
          ({"mean": None}, b"null"), ({"x": None}, b"null"), ({"y": None}, b"null"), ({"loss": None}, b"null"),
          ({"sq": None}, b"null"), ({"dev": None}, b"null deviation"), ({"k": 0}, b"k 0"), ({"frequency": 0}, b"frequency"),
          ({"col": 1}, b"deviation column"), ({"n": 3, "slot0": 4}, b"did not start at count 0")]


ERROR_CALLS = [(name, over, message) for name in sorted(NAMES) for over, message in ERRORS
               if set(over) <= set(PARAMS[name]) and ("slot0" not in over or "swag" in name)]


@pytest.mark.parametrize("name,over,message", ERROR_CALLS, ids=[f"{n}-{'-'.join(o) or 'plan'}" for n, o, _ in ERROR_CALLS])
def test_argument_errors_are_refused_without_a_gpu(name, over, message):
    lib = _lib.load()
    args, _keep = call_args(name, **over)
    assert getattr(lib, name)(*args) == -1                               # PYZ_E_INVALID
    err = lib.pyz_last_error()
    assert err and message in err, err


# ---------------------------------------------------------------- Mixture
def lowrank(mean_value, size=6, k=2):
    from bayesian_inference_for_nn_amd.distributions import MultivariateNormalDiagPlusLowRank
    return MultivariateNormalDiagPlusLowRank(np.full(size, mean_value, dtype=np.float32), np.full(size, 1e-3, dtype=np.float32),
                                             np.zeros((size, k), dtype=np.float32))


def test_mixture_indices_follow_the_frequencies_by_sampled_rule():
    from bayesian_inference_for_nn_amd.distributions import Mixture, Sampled
    freqs = [1, 3, 2]
    mix = Mixture([lowrank(-100.0), lowrank(0.0), lowrank(100.0)], freqs)
    random.seed(5)
    idx = [mix.sample_index() for _ in range(200)]
    ref = Sampled([np.zeros(6, dtype=np.float32)] * 3, freqs)
    random.seed(5)
    assert idx == [ref.sample_index() for _ in range(200)]
    counts = np.bincount(idx, minlength=3)
    assert counts.sum() == 200 and counts[1] > counts[2] > counts[0] > 0
    assert Mixture([lowrank(0.0), lowrank(1.0)])._frequencies == [1, 1]   # default: all 1


def test_mixture_rows_come_from_the_drawn_component():
    from bayesian_inference_for_nn_amd.distributions import Mixture
    mix = Mixture([lowrank(-100.0), lowrank(100.0)], [2, 1])
    random.seed(11)
    rows = mix.sample_n(40)
    random.seed(11)
    idx = [mix.sample_index() for _ in range(40)]
    assert rows.shape == (40, 6) and rows.dtype == np.float32 and 0 < sum(idx) < 40
    for r, c in enumerate(idx):
        assert np.all(np.abs(rows[r] - (-100.0, 100.0)[c]) < 0.1), (r, c, rows[r])
    one = mix.sample()
    assert one.shape == (6,) and np.all(np.abs(np.abs(one) - 100.0) < 0.1)


def test_mixture_store_load_inside_a_bayesian_model(tmp_path):
    from bayesian_inference_for_nn_amd.distributions import Mixture
    from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json
    cfg = sequential_json(2, [3, 2], ["tanh", "softmax"])
    model = BayesianModel(cfg)
    D = model._model.spec.n_params
    rng = np.random.default_rng(3)
    from bayesian_inference_for_nn_amd.distributions import MultivariateNormalDiagPlusLowRank as LowRank
    comps = [LowRank(rng.normal(size=D).astype(np.float32), rng.uniform(0.1, 1.0, size=D).astype(np.float32),
                     rng.normal(size=(D, 3)).astype(np.float32)) for _ in range(3)]
    model.apply_distribution(Mixture(comps, [4, 1, 2]), 0, len(model._model.layers) - 1)
    model.store(str(tmp_path / "m"))
    assert os.path.exists(tmp_path / "m" / "distribution0" / "mixture.json")
    assert os.path.isdir(tmp_path / "m" / "distribution0" / "component2")
    back = BayesianModel.load(str(tmp_path / "m"))
    assert back._layers_dtbn_intervals == [[0, len(model._model.layers) - 1]]
    mix = back._distributions[0]
    assert isinstance(mix, Mixture) and mix._frequencies == [4, 1, 2] and mix.size == D and len(mix.components) == 3
    for a, b in zip(comps, mix.components):
        assert isinstance(b, LowRank)
        for attr in ("_mean", "_diag", "_D"):
            x, y = getattr(a, attr), getattr(b, attr)
            assert x.dtype == y.dtype == np.float32 and x.shape == y.shape and x.tobytes() == y.tobytes(), attr
    draws = back.sample_weights_matrix(5)
    assert draws.shape == (5, D) and np.all(np.isfinite(draws))


def test_mixture_refuses_unequal_sizes_and_zero_frequencies():
    from bayesian_inference_for_nn_amd.distributions import Mixture
    with pytest.raises(ValueError):
        Mixture([lowrank(0.0, size=6), lowrank(0.0, size=7)])
    with pytest.raises(ValueError):
        Mixture([lowrank(0.0), lowrank(1.0)], [1, 0])
    with pytest.raises(ValueError):
        Mixture([lowrank(0.0), lowrank(1.0)], [1])
    with pytest.raises(ValueError):
        Mixture([])


def test_mixture_is_exported():
    import bayesian_inference_for_nn_amd.distributions as d
    assert d.Mixture.__name__ == "Mixture"
    import sys
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        from Pyesian.distributions import Mixture
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    assert Mixture is d.Mixture


# ---------------------------------------------------------------- the optimizer surface before any device work
@pytest.mark.parametrize("which", ["SGD", "SWAG"])
def test_starting_model_list_of_the_wrong_length_raises_before_any_device_work(which, monkeypatch):
    from bayesian_inference_for_nn_amd import optimizers, synth
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import MeanSquaredError
    from bayesian_inference_for_nn_amd.nn import sequential_json
    from bayesian_inference_for_nn_amd.nn.model import model_from_json
    from bayesian_inference_for_nn_amd.optimizers.Optimizer import Optimizer
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

    def no_device(self, *a, **kw):
        raise AssertionError("the backend was set up before the starting models were checked")
    monkeypatch.setattr(Optimizer, "_setup_backend", no_device)
    x, y = synth.linreg(70)
    cfg = sequential_json(1, [5, 1], ["tanh", "linear"])
    ds = Dataset((x / 20.0, y / 40.0), MeanSquaredError, "Regression", seed=0)
    hp = HyperParameters(lr=0.01, frequency=2, k=3, scale=1.0, batch_size=16)
    starts = [model_from_json(cfg), model_from_json(cfg)]
    with pytest.raises(ValueError, match="starting_model"):
        getattr(optimizers, which)().compile(hp, cfg, ds, verbose=False, seed=1, n_members=3, starting_model=starts)
    with pytest.raises(ValueError, match="n_members"):
        getattr(optimizers, which)().compile(hp, cfg, ds, verbose=False, seed=1, n_members=0, starting_model=starts[0])
