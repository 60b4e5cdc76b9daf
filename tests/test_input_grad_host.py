"""CPU checks of the input gradient (pyz_input_grad, Robustness.adversarial_robustness): the C-ABI entry point, the float64
restatement the device tests compare against (tests/input_grad_checks.py) pinned to torch autograd, what the case table
reaches, the cap on the elements whose sign the device tests leave open, and the host logic of Robustness."""

import os
import re
import sys

import numpy as np
import pytest
import torch

from dense_cases import can_fuse
from input_grad_checks import (CASES, EXCLUDE_CAP, accuracy, case_ref, chunks, fgsm, input_grad_ref, input_grad_vec,
                               input_grad_waves, rmse, sign_stable, surface_classification, surface_regression)
from oracle import mlp as o_mlp

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.losses import MeanSquaredError, SparseCategoricalCrossentropy
from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json
from bayesian_inference_for_nn_amd.visualisations import Robustness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"pyz_mlp *": _lib._p, "const float *": _lib._p, "const void *": _lib._p, "float *": _lib._p, "void *": _lib._p,
         "int": _lib.C.c_int, "float": _lib._f}


def test_entry_point_is_declared_with_matching_argument_types():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pyz.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+pyz_input_grad\s*\(([^)]*)\)\s*;", src)
    assert proto, "pyz_input_grad is not declared in include/pyz.h"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    types = [re.sub(r"\s*\w+$", "", p) if not p.endswith("*") else p for p in params]
    types = [t if not t.endswith("*") else t[:-1].strip() + " *" for t in types]
    restype, argtypes = _lib.SIGNATURES["pyz_input_grad"]
    assert restype is _lib.C.c_int
    assert [CTYPE[t] for t in types] == list(argtypes) and len(argtypes) == 12
    assert hasattr(_lib.load(), "pyz_input_grad")
    assert _lib.header_version() == 302


def test_null_plan_is_refused_without_a_gpu():
    lib = _lib.load()
    rc = lib.pyz_input_grad(None, None, 1, None, None, 1, 1.0, None, 0.1, None, None, None)
    assert rc < 0 and b"null plan" in lib.pyz_last_error()


def _torch_grad(thetas, x, y, spec):
    """d (sum over draws of the mean loss) / d x by torch float64 autograd."""
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    total = 0.0
    fn = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "linear": lambda z: z, "softmax": lambda z: z}
    for theta in thetas:
        h = xt
        for (w, b), a in zip(o_mlp.unpack(np.asarray(theta, dtype=np.float64), spec), spec.acts):
            h = fn[a](h @ torch.tensor(w) + torch.tensor(b))
        if spec.loss == "scce":
            total = total + torch.nn.functional.cross_entropy(h, torch.tensor(np.asarray(y), dtype=torch.long))
        else:
            total = total + ((h - torch.tensor(np.asarray(y, dtype=np.float64))) ** 2).mean(dim=-1).mean()
    total.backward()
    return xt.grad.numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_restatement_equals_torch_autograd(case):
    x, y, thetas, G, losses = case_ref(case)
    want = _torch_grad(thetas, x, y, case.spec)
    assert np.abs(G - want).max() <= 1e-10 * np.abs(want).max()
    assert np.isfinite(losses).all() and len(losses) == case.draws
    half, _ = input_grad_ref(thetas, x, y, case.spec, scale=0.5)
    np.testing.assert_array_equal(half, 0.5 * G)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_gradient_keeps_the_exclusion_cap(case):
    """The device tests leave the sign of the elements below 1e-3 of the largest open; they may be 3 % at most."""
    G = case_ref(case)[3]
    assert 1.0 - sign_stable(G).mean() <= EXCLUDE_CAP
    assert np.abs(G).max() > 0.0


def test_surface_data_meets_what_the_device_tests_assume():
    """The device tests of the surface hold the device to the restatement's verdict: the attack lowers the score at the
    test's epsilon, and the reference gradient keeps the exclusion cap there too."""
    c, r = surface_classification(), surface_regression()
    for s in (c, r):
        assert 1.0 - sign_stable(s.G).mean() <= EXCLUDE_CAP
    assert len(c.xv) == 30 and accuracy(c, c.xv) == 100.0 and accuracy(c, fgsm(c.xv, c.G, c.eps)) < 100.0
    assert len(r.xv) == 20 and rmse(r, fgsm(r.xv, r.G, r.eps)) > rmse(r, r.xv)
    print(accuracy(c, fgsm(c.xv, c.G, c.eps)), rmse(r, r.xv), rmse(r, fgsm(r.xv, r.G, r.eps)),
          1.0 - sign_stable(c.G).mean(), 1.0 - sign_stable(r.G).mean())


def test_case_table_reaches_every_wave_count_both_operand_paths_and_chunked_draws():
    seen_S, seen_vec, chunked, fused, layers, losses = set(), set(), False, set(), set(), set()
    for c in CASES:
        la = c.launches()
        assert sum(P for P, _, _ in la) == c.draws and all(P <= c.max_p for P, _, _ in la)
        chunked |= len(la) > 1
        fused.add(can_fuse(c.dims))
        layers.add(min(len(c.dims) - 1, 3))
        losses.add(c.loss)
        for P, S, vec in la:
            seen_S.add(S)
            seen_vec.add((vec, S > 1))
    assert seen_S == {1, 2, 4, 8, 16}
    assert seen_vec == {(0, False), (0, True), (1, False), (1, True)}   # dword and float4 steps, one wave and several
    assert chunked and fused == {True, False} and layers == {1, 2, 3} and losses == {"scce", "mse"}
    by = {c.name: c for c in CASES}
    assert [s for _, s, _ in by["wide_p3"].launches()] == [8] and [s for _, s, _ in by["wide_p4"].launches()] == [16]
    assert by["vec_on"].launches()[0][2] == 1 and by["vec_off_odd_d"].launches()[0][2] == 0
    assert by["wide_p4_vec"].launches() == [(4, 16, 1)]
    assert [P for P, _, _ in by["deep"].launches()] == [3, 3, 1]
    # the rule itself at its edges
    assert chunks(7, 3) == [(0, 3), (3, 3), (6, 1)] and chunks(2, 5) == [(0, 2)]
    assert input_grad_vec(16, 1, 659, 0) == 1 and input_grad_vec(16, 1, 659, 1) == 0 and input_grad_vec(16, 2, 659, 0) == 0
    assert input_grad_vec(12, 1, 8, 0) == 0 and input_grad_vec(16, 3, 676, 3) == 1
    assert input_grad_waves(6000, 784, 200, 100) == 1          # the MNIST shape: 4 700 tiles fill the chip on their own


def test_launch_rules_restate_the_source():
    api = open(os.path.join(ROOT, "bayesian_inference_for_nn_amd", "csrc", "pyz_api.hip")).read()
    hdr = open(os.path.join(ROOT, "bayesian_inference_for_nn_amd", "csrc", "pyz_input_grad.h")).read()
    assert "const int S = pyz_pick_waves(tiles, (long long)g.P * g.N / 2);" in hdr
    assert "const long long tiles = (long long)((g.rows + 31) / 32) * ((g.K + 31) / 32);" in hdr
    assert ("g.vec = (N % 8 == 0) && (m->w_off[0] % 4 == 0) && (P == 1 || m->D % 4 == 0) && aligned16(theta) ? 1 : 0;"
            in api)
    assert "const int chunk = std::min(m->max_p, pyz_input_grad_max_draws(N));" in api
    assert '#include "pyz_input_grad.h"' in api


def test_fgsm_restatement_keeps_zero_and_nan():
    x = np.array([1.0, 2.0, 3.0, 4.0], dtype=np.float32)
    out = fgsm(x, np.array([0.5, -2.0, 0.0, np.nan]), 0.25)
    np.testing.assert_array_equal(out[:3], np.array([1.25, 1.75, 3.0], dtype=np.float32))
    assert np.isnan(out[3])


# ---------------------------------------------------------------- Robustness (host logic)
def _patched(monkeypatch, bm, x_adv, mean, calls):
    def adversarial_examples(x, y, loss, epsilon, nb_samples):
        calls.append(("adv", np.asarray(x).shape, np.asarray(y).shape, loss, epsilon, nb_samples))
        return x_adv, np.zeros_like(x_adv)

    def predict(x, nb_samples):
        calls.append(("predict", x is x_adv, nb_samples))
        return [mean], mean

    monkeypatch.setattr(bm, "adversarial_examples", adversarial_examples, raising=True)
    monkeypatch.setattr(bm, "predict", predict, raising=True)


def test_robustness_classification_scoring_print_and_file(monkeypatch, capsys, tmp_path):
    rng = np.random.default_rng(0)
    x, y = rng.normal(size=(80, 4)).astype(np.float32), rng.integers(0, 3, size=80)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=1)
    bm = BayesianModel(sequential_json(4, [5, 3], ["relu", "softmax"]))
    xv, yv = ds.valid_data.as_numpy()
    assert len(xv) == 8
    mean = np.full((8, 3), 0.1)
    right = [0, 1, 2, 4, 7]
    for i in range(8):
        mean[i, yv[i] if i in right else (yv[i] + 1) % 3] = 0.8
    calls = []
    x_adv = xv + 1.0
    _patched(monkeypatch, bm, x_adv, mean, calls)
    rb = Robustness((bm, "history"), ds)          # a result() tuple
    v = rb.adversarial_robustness(epsilon=0.2, nb_samples=7)
    assert v == 5 / 8 * 100
    assert capsys.readouterr().out == "Adversarial Robustness: 62.5%\n"
    assert calls == [("adv", (8, 4), (8,), "scce", 0.2, 7), ("predict", True, 7)]
    v2 = Robustness(bm, ds).adversarial_robustness(save_path=str(tmp_path))
    assert capsys.readouterr().out == ""
    path = tmp_path / "report" / "robustness" / "adversarial_robustness.txt"
    assert path.read_text() == str(v2) == "62.5"
    assert calls[2][4:] == (0.1, 100) and calls[3] == ("predict", True, 100)      # the defaults of the reference


def test_robustness_regression_scores_rmse(monkeypatch, capsys, tmp_path):
    rng = np.random.default_rng(1)
    x, y = rng.normal(size=(50, 3)).astype(np.float32), rng.normal(size=(50, 2)).astype(np.float32)
    ds = Dataset((x, y), MeanSquaredError, "Regression", target_dim=2, seed=2)
    bm = BayesianModel(sequential_json(3, [4, 2], ["tanh", "linear"]))
    xv, yv = ds.valid_data.as_numpy()
    mean = yv.reshape(len(xv), 2).astype(np.float64) + np.array([3.0, 4.0])
    calls = []
    _patched(monkeypatch, bm, xv.copy(), mean, calls)
    v = Robustness(bm, ds).adversarial_robustness(epsilon=0.05, nb_samples=3)
    assert v == pytest.approx(3.5, rel=1e-12)           # per-column RMSE 3 and 4, averaged
    assert capsys.readouterr().out == "Adversarial Robustness: " + str(v) + "\n"
    assert calls[0][3:] == ("mse", 0.05, 3)
    Robustness(bm, ds).adversarial_robustness(save_path=str(tmp_path))
    assert (tmp_path / "report" / "robustness" / "adversarial_robustness.txt").read_text() == str(v)


def test_unsupported_combinations_raise_value_error():
    bm = BayesianModel(sequential_json(3, [4, 2], ["tanh", "linear"]))
    x, y = np.zeros((4, 3), dtype=np.float32), np.zeros(4, dtype=np.int32)
    with pytest.raises(ValueError):
        bm.adversarial_examples(x, y, "scce", 0.1, 2)              # scce without a softmax last layer
    with pytest.raises(ValueError):
        bm.adversarial_examples(x, y, "hinge", 0.1, 2)
    bm2 = BayesianModel(sequential_json(3, [4, 2], ["tanh", "softmax"]))
    with pytest.raises(ValueError):
        bm2.adversarial_examples(x, np.zeros((4, 2), dtype=np.float32), "mse", 0.1, 2)


def test_class_is_reexported_by_compat_beside_the_stand_ins():
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import Pyesian.visualisations as cv
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    assert cv.Robustness is Robustness and hasattr(cv, "Metrics") and hasattr(cv, "Plotter")
    assert not hasattr(Robustness, "mean_corruption_error")       # no stubs for the host-side corruption measures
