#!/usr/bin/env python3
"""Cost of Robustness.mean_corruption_error at the size of the reference's driver (GPU box): 784 -> 256 -> 256 -> 10, grey
28 x 28 rows of a synthetic MNIST-shaped data set (synth.mnist_like), 100 weight draws of a Normal posterior, nine
corruptions x five severities = 45 read-outs of the split.
    mean_corruption_error_ms  the whole call on a fresh Robustness (every corruption a cache miss; wall clock, median of
                              --rounds after one warm-up call that builds the plan)
    kernels                   {kernel: [launches, mean us]} of one such call (KernelProbe), and their total
    k_corrupt_rows            per measured kind (a noise kind and the blur): us of the five-severity launch, the bytes it
                              moves (reads rows * 784 floats, writes 5 * rows * 784), bytes / s and the fraction of the 6.3 TB/s
                              achievable HBM rate
    host_baseline             the same 45 error rates with the corrupted rows made on the HOST by the NumPy functions of
                              tests/corruption_checks.py (float64, the library's Philox stream restated in NumPy), uploaded
                              and read out with BayesianModel.predictive_mean, NumPy argmax; wall clock of one pass, with
                              the share spent making the rows.  It is a vectorised stand-in, NOT the reference's per-image
                              Python loop through PIL and skimage
Prints one JSON line."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import corruption_checks as cc  # noqa: E402
from bayesian_inference_for_nn_amd import engine, synth  # noqa: E402
from bayesian_inference_for_nn_amd.datasets import Dataset  # noqa: E402
from bayesian_inference_for_nn_amd.distributions import tfd  # noqa: E402
from bayesian_inference_for_nn_amd.distributions.tf import TensorflowProbabilityDistribution  # noqa: E402
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy  # noqa: E402
from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json  # noqa: E402
from bayesian_inference_for_nn_amd.visualisations import Robustness  # noqa: E402

DIMS, ACTS = (784, 256, 256, 10), ("relu", "relu", "softmax")
DRAWS, SEED = 100, 5
HBM_TBS = 6.3            # achievable HBM rate
SEV = [1, 2, 3, 4, 5]


def _quiet(fn):
    out, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        return fn()
    finally:
        sys.stdout.close()
        sys.stdout = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_corruption.py needs the GPU"
    x, y = synth.mnist_like(args.rows, seed=1234)
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(args.rows, 28, 28))
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", train_proportion=0.0, test_proportion=0.0,
                 valid_proportion=1.0, seed=0)
    bm = BayesianModel(sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS)))
    loc = synth.glorot_uniform(DIMS).astype(np.float32)
    bm.apply_distribution(TensorflowProbabilityDistribution(tfd.Normal(loc, np.full_like(loc, 0.02))), 0, len(ACTS) - 1)
    xv, yv = ds.valid_data.as_numpy()
    n = len(xv)
    pixel_max = 255.0 if float(np.max(xv)) > 1.0 else 1.0
    tfd.seed(3)

    wall = []
    for i in range(args.rounds + 1):         # the first call builds the model's plan
        rb = Robustness(bm, ds, pixel_max=pixel_max, seed=SEED)      # a fresh cache: every corruption is a miss
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mce = _quiet(lambda: rb.mean_corruption_error(nb_samples=DRAWS))
        if i:
            wall.append((time.perf_counter() - t0) * 1e3)
    rb = Robustness(bm, ds, pixel_max=pixel_max, seed=SEED)
    with engine.KernelProbe(4096) as kp:
        _quiet(lambda: rb.mean_corruption_error(nb_samples=DRAWS))
    split = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}

    xd = torch.as_tensor(np.ascontiguousarray(xv.reshape(n, -1), dtype=np.float32)).cuda()
    nbytes = 4.0 * (n * 784 + 5 * n * 784)
    rates = {}
    for kind in (cc.GAUSS, cc.BLUR):
        for _ in range(3):
            engine.corrupt_rows(xd, (28, 28, 1), kind, SEV, pixel_max=pixel_max, seed=SEED)
        us = []
        for _ in range(max(5, args.rounds)):
            with engine.KernelProbe(8) as k1:
                engine.corrupt_rows(xd, (28, 28, 1), kind, SEV, pixel_max=pixel_max, seed=SEED)
            us.append(sum(t for name, t in k1.launches if name == "k_corrupt_rows"))
        med = float(np.median(us))
        tbs = nbytes / (med * 1e-6) / 1e12
        rates[cc.NAMES[kind]] = {"us": round(med, 1), "us_rounds": [round(v, 1) for v in us], "mbytes": round(nbytes / 1e6, 1),
                                 "tb_per_s": round(tbs, 3), "hbm_tb_per_s": HBM_TBS, "fraction_of_hbm": round(tbs / HBM_TBS, 4)}

    res = {"tool": "bench_corruption", "shape": "784-256-256-10", "rows": n, "image": "28x28x1", "draws": DRAWS,
           "rounds": args.rounds, "pixel_max": pixel_max, "mean_corruption_error": round(mce, 4),
           "mean_corruption_error_ms": round(float(np.median(wall)), 2),
           "mean_corruption_error_ms_rounds": [round(v, 2) for v in wall], "kernels": split,
           "kernel_us_total": round(sum(t for _, t in kp.launches), 1), "k_corrupt_rows": rates}

    if not args.no_baseline:
        x4 = np.asarray(xv, dtype=np.float32).reshape(n, 28, 28, 1)
        labels = np.asarray(yv).reshape(-1)
        t_all = time.perf_counter()
        t_rows, errors = 0.0, []
        for kind in range(9):
            frac = []
            for sev in SEV:
                t0 = time.perf_counter()
                rows = cc.finish(cc.corrupt(x4, kind, sev, pixel_max, SEED)["value"], 1, pixel_max, True, dtype=np.float32)
                t_rows += time.perf_counter() - t0
                mean = bm.predictive_mean(rows, DRAWS)
                frac.append(float((mean.argmax(axis=1) != labels).mean()))
            errors.append(np.sum(np.array(frac) * 100) / 5)
            print(f"[bench_corruption] host baseline: {cc.NAMES[kind]} done", file=sys.stderr, flush=True)
        total = (time.perf_counter() - t_all) * 1e3
        res["host_baseline"] = {"ms": round(total, 1), "ms_making_rows": round(t_rows * 1e3, 1),
                                "mean_corruption_error": round(float(np.mean(errors)), 4),
                                "kind": "rows corrupted by the float64 NumPy restatements (tests/corruption_checks.py), uploaded, "
                                        "BayesianModel.predictive_mean, NumPy argmax (not the reference's per-image PIL / "
                                        "skimage loop)"}
        res["speedup_vs_host_baseline"] = round(total / res["mean_corruption_error_ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
