#!/usr/bin/env python3
"""Cost of Metrics.classification_uncertainty at the MNIST shape (GPU box): 784 -> 200 -> 10, 10 000 rows of a synthetic
MNIST-shaped data set (synth.mnist_like), 100 weight draws of a Normal posterior.
    predict_moments_ms     pyz_predict_moments (forward of every draw + k_predict_moments; device events, median of --rounds)
    predict_ms             pyz_predict with the sample tensor, the same way (what the moments replace on the device)
    kernels                {kernel: [launches, mean us]} of one pyz_predict_moments call (KernelProbe)
    k_predict_moments      its time, the bytes it moves (reads draws * rows * C floats, writes rows * (C + C * C)), bytes / s
                           and the fraction of the 6.3 TB/s achievable HBM rate
    uncertainty_ms         the whole Metrics.classification_uncertainty call on a cache miss (weight draws, moments, download
                           of 4.4 MB, the closed forms in NumPy; wall clock, median of --rounds)
    einsum_baseline        the same three arrays from BayesianModel.predict's HOST samples (the 40 MB download included) and a
                           NumPy einsum for the second moment; wall clock.  It is a vectorised stand-in, NOT the reference's
                           Python loop over every draw and row (a million small TensorFlow calls at this size)
Prints one JSON line."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bayesian_inference_for_nn_amd import engine, synth  # noqa: E402
from bayesian_inference_for_nn_amd.datasets import Dataset  # noqa: E402
from bayesian_inference_for_nn_amd.distributions import tfd  # noqa: E402
from bayesian_inference_for_nn_amd.distributions.tf import TensorflowProbabilityDistribution  # noqa: E402
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy  # noqa: E402
from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json  # noqa: E402
from bayesian_inference_for_nn_amd.visualisations import Metrics  # noqa: E402
from bayesian_inference_for_nn_amd.visualisations.Metrics import uncertainty_from_moments  # noqa: E402

DIMS, ACTS = (784, 200, 10), ("relu", "softmax")
ROWS, DRAWS = 10_000, 100
HBM_TBS = 6.3            # achievable HBM rate


def _events(fn, rounds):
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics.py needs the GPU"
    x, y = synth.mnist_like(ROWS, seed=1234)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", train_proportion=0.0, test_proportion=1.0,
                 valid_proportion=0.0, seed=0)
    bm = BayesianModel(sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS)))
    loc = synth.glorot_uniform(DIMS).astype(np.float32)
    bm.apply_distribution(TensorflowProbabilityDistribution(tfd.Normal(loc, np.full_like(loc, 0.02))), 0, 1)
    xt, yt = ds.test_data.as_numpy()
    xt = np.ascontiguousarray(xt.reshape(len(xt), -1), dtype=np.float32)
    n, C = len(xt), DIMS[-1]
    tfd.seed(3)
    Wd = bm.sample_weights_device(DRAWS)
    xd = torch.as_tensor(xt).cuda()
    plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=n, max_particles=DRAWS)
    for _ in range(2):
        plan.predict_moments(Wd, xd)
        plan.predict(Wd, xd)
    torch.cuda.synchronize()
    ms = _events(lambda: plan.predict_moments(Wd, xd), args.rounds)
    ms_predict = _events(lambda: plan.predict(Wd, xd), args.rounds)
    with engine.KernelProbe(64) as kp:
        plan.predict_moments(Wd, xd)
    split = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}
    pm_us = sum(t for name, t in kp.launches if name == "k_predict_moments")
    nbytes = 4.0 * (DRAWS * n * C + n * (C + C * C))
    tbs = nbytes / (pm_us * 1e-6) / 1e12
    with engine.KernelProbe(64) as kp2:
        plan.predict(Wd, xd)
    split_predict = {name: [c, round(t, 2)] for name, (c, t) in kp2.by_kernel().items()}

    devnull = open(os.devnull, "w")
    wall, base = [], []
    for i in range(args.rounds + 1):       # the first call builds the model's plan
        m = Metrics(bm, ds)                # a fresh cache: every call is a miss
        out, sys.stdout = sys.stdout, devnull
        try:
            t0 = time.perf_counter()
            got = m.classification_uncertainty(n_boundaries=DRAWS, n_samples=n)
            dt = time.perf_counter() - t0
            t0 = time.perf_counter()
            samples, _ = bm.predict(xt, DRAWS)
            p = np.asarray(samples, dtype=np.float64)
            want = uncertainty_from_moments(p.mean(axis=0), np.einsum("sja,sjb->jab", p, p), DRAWS, n)
            db = time.perf_counter() - t0
        finally:
            sys.stdout = out
        if i:
            wall.append(dt * 1e3)
            base.append(db * 1e3)
    assert got[0].shape == want[0].shape == (n, C, C)

    res = {"tool": "bench_metrics", "shape": "784-200-10", "rows": n, "draws": DRAWS, "rounds": args.rounds,
           "predict_moments_ms": round(float(np.median(ms)), 3), "predict_moments_ms_rounds": [round(v, 3) for v in ms],
           "predict_ms": round(float(np.median(ms_predict)), 3), "kernels": split, "kernels_predict": split_predict,
           "kernel_us_total": round(sum(t for _, t in kp.launches), 1),
           "k_predict_moments": {"us": round(pm_us, 1), "mbytes": round(nbytes / 1e6, 1), "tb_per_s": round(tbs, 3),
                                 "hbm_tb_per_s": HBM_TBS, "fraction_of_hbm": round(tbs / HBM_TBS, 4)},
           "uncertainty_ms": round(float(np.median(wall)), 2), "uncertainty_ms_rounds": [round(v, 2) for v in wall],
           "einsum_baseline": {"ms": round(float(np.median(base)), 1), "ms_rounds": [round(v, 1) for v in base],
                               "kind": "BayesianModel.predict's host samples + NumPy float64 einsum (not the reference's "
                                       "per-draw, per-row Python loop)"},
           }
    res["speedup_uncertainty_vs_einsum"] = round(res["einsum_baseline"]["ms"] / res["uncertainty_ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
