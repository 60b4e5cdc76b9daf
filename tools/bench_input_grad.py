#!/usr/bin/env python3
"""Cost of the adversarial-robustness evaluation at the MNIST shape (GPU box): 784 -> 200 -> 10, the 6 000 validation
rows of a 60 000-row synthetic MNIST-shaped data set (synth.mnist_like), 100 weight draws of a Normal posterior.
    input_grad_ms          pyz_input_grad (gradient, FGSM step and per-draw losses; device events, median of --rounds)
    robustness_ms          the whole Robustness.adversarial_robustness call (weight draws, input gradient, download,
                           Monte-Carlo prediction on the perturbed rows, scoring; wall clock, median of --rounds)
    kernels                {kernel: [launches, mean us]} of one pyz_input_grad call (KernelProbe)
    k_input_grad           its time, 2 * rows * 784 * draws * 200 flop / time in TFLOP/s and the fraction of the 157.3
                           TFLOP/s fp32-MFMA peak
    cpu_baseline           the same quantity -- the input gradient summed over the draws -- by eager torch autograd on the
                           host (float32, 16 threads at most), timed on a bounded sample of draws and scaled to all of them
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
from bayesian_inference_for_nn_amd.visualisations import Robustness  # noqa: E402

DIMS, ACTS = (784, 200, 10), ("relu", "softmax")
N_ROWS, DRAWS, EPSILON = 60_000, 100, 0.1
PEAK_TFLOPS = 157.3      # fp32 MFMA, the roofline figure of DESIGN.md


def cpu_baseline(x, y, thetas, budget_s=12.0):
    """Eager torch autograd of the mean loss with respect to x, one tape per draw as the reference runs it."""
    from bench import cpu_model, host_cores
    cores = min(host_cores(), 16)
    torch.set_num_threads(cores)
    xt = torch.as_tensor(x).requires_grad_(True)
    yt = torch.as_tensor(y.astype(np.int64))
    K, H, C = DIMS
    total = torch.zeros_like(xt)

    def one(theta):
        t = torch.as_tensor(theta)
        w0, b0 = t[:K * H].view(K, H), t[K * H:K * H + H]
        o = K * H + H
        w1, b1 = t[o:o + H * C].view(H, C), t[o + H * C:]
        loss = torch.nn.functional.cross_entropy(torch.relu(xt @ w0 + b0) @ w1 + b1, yt)
        g, = torch.autograd.grad(loss, xt)
        total.add_(g)

    one(thetas[0])
    t0, n = time.perf_counter(), 0
    while (time.perf_counter() - t0 < budget_s or n < 4) and n < len(thetas):
        one(thetas[n])
        n += 1
    dt = time.perf_counter() - t0
    return {"ms_per_draw": round(dt / n * 1e3, 2), "ms_all_draws": round(dt / n * len(thetas) * 1e3, 1), "draws_timed": n,
            "cores": cores, "cpu_model": cpu_model(), "kind": "port",
            "sample": f"{n} of {len(thetas)} draws: eager torch-CPU autograd (fp32) of the mean loss over {len(x)} rows with "
                      "respect to the inputs; TensorFlow is not installed"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_input_grad.py needs the GPU"
    x, y = synth.mnist_like(N_ROWS, seed=1234)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=0)
    bm = BayesianModel(sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS)))
    loc = synth.glorot_uniform(DIMS).astype(np.float32)
    bm.apply_distribution(TensorflowProbabilityDistribution(tfd.Normal(loc, np.full_like(loc, 0.02))), 0, 1)
    xv, yv = ds.valid_data.as_numpy()
    xv = np.ascontiguousarray(xv.reshape(len(xv), -1), dtype=np.float32)
    n = len(xv)
    tfd.seed(3)
    Wd = bm.sample_weights_device(DRAWS)
    xd, yd = torch.as_tensor(xv).cuda(), torch.as_tensor(yv.astype(np.int32)).cuda()
    plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=n, max_particles=DRAWS)

    for _ in range(2):
        plan.input_grad(Wd, xd, yd, epsilon=EPSILON)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.input_grad(Wd, xd, yd, epsilon=EPSILON)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    with engine.KernelProbe(64) as kp:
        plan.input_grad(Wd, xd, yd, epsilon=EPSILON)
    plan.check_finite()
    split = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}
    ig_us = sum(t for name, t in kp.launches if name == "k_input_grad")
    flop = 2.0 * n * DIMS[0] * DRAWS * DIMS[1]
    tflops = flop / (ig_us * 1e-6) / 1e12

    rb = Robustness(bm, ds)
    devnull = open(os.devnull, "w")
    wall, score = [], None
    for i in range(args.rounds + 1):       # the first call builds the plans
        out, sys.stdout = sys.stdout, devnull
        try:
            t0 = time.perf_counter()
            score = rb.adversarial_robustness(epsilon=EPSILON, nb_samples=DRAWS)
            dt = time.perf_counter() - t0
        finally:
            sys.stdout = out
        if i:
            wall.append(dt * 1e3)

    res = {"tool": "bench_input_grad", "shape": "784-200-10", "rows": n, "draws": DRAWS, "epsilon": EPSILON,
           "rounds": args.rounds, "input_grad_ms": round(float(np.median(ms)), 3),
           "input_grad_ms_rounds": [round(v, 3) for v in ms],
           "robustness_ms": round(float(np.median(wall)), 2), "robustness_ms_rounds": [round(v, 2) for v in wall],
           "robustness_score": score, "kernels": split,
           "kernel_us_total": round(sum(t for _, t in kp.launches), 1),
           "k_input_grad": {"us": round(ig_us, 1), "gflop": round(flop / 1e9, 1), "tflops": round(tflops, 2),
                            "peak_tflops": PEAK_TFLOPS, "fraction_of_peak": round(tflops / PEAK_TFLOPS, 4)}}
    if not args.no_cpu:
        res["cpu_baseline"] = cpu_baseline(xv, yv, Wd.cpu().numpy())
        res["speedup_input_grad_vs_cpu"] = round(res["cpu_baseline"]["ms_all_draws"] / res["input_grad_ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
