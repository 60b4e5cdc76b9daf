#!/usr/bin/env python3
"""Cost of a Bayes-by-Backprop hyper-parameter grid on BBB lanes against the same grid point by point, at the C4 shape (GPU
box): 784 -> 400 -> 400 -> 10, batch 1024, synthetic MNIST-shaped rows (synth.mnist_like) with 7 * 1024 + 896 rows in the
training split, so every eighth batch is the ragged 896-row one.  The grid: 8 values of lr x 4 of alpha = 32 points, --steps
(default 200) BBB steps each, scored by the misclassified fraction of the posterior means on the validation split.
    lanes    GridOptimizer + BBBGridObjective(max_lanes=32, weights="mu"): ONE BBB compiled with 32 lanes, one quiet train
             (pyz_bbb_lanes_run), one lane_scores (pyz_lane_scores)
    serial   the reference's loop: per point a BBB compiled with the point's hyper-parameters, a quiet single train
             (pyz_bbb_run, with its validation forward), the validation split through plan.predict of mu, the (rows, 10)
             probabilities to the host and the error count there
Both legs start every training from the same seed.  The legs alternate inside one process; each is timed as a whole (wall
clock, it ends with its scores on the host) and split into compile / train / score; the figures are medians of --rounds
rounds and `rounds_ms` keeps every round.  `kernels`: {kernel: [launches, mean us]} of 8 steps of the 32-lane step and of 8
single pyz_bbb_step calls beside it under KernelProbe (twice: a process's kernels get faster over its first launches);
`streaming`: the two new kernels alone -- the bytes they move (sample: mu, rho read and w written; update: mu, rho, w, grad
read and mu, rho written; 32 lanes x D floats each), bytes / s and the fraction of the 6.3 TB/s achievable HBM rate.
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
from bayesian_inference_for_nn_amd.distributions import GaussianPrior  # noqa: E402
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy  # noqa: E402
from bayesian_inference_for_nn_amd.nn import sequential_json  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers import BBB  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import BBBGridObjective, GridOptimizer, HyperParameters, Real  # noqa: E402

DIMS, ACTS = (784, 400, 400, 10), ("relu", "relu", "softmax")
BATCH, N_ROWS = 1024, 7 * 1024 + 896
BASE = dict(lr=1e-3, alpha=1e-4, batch_size=BATCH)
LRS = [5e-4 * (i + 1) for i in range(8)]
ALPHAS = [1e-5, 1e-4, 1e-3, 1e-2]
PRIOR = (0.0, -5.0)      # mean and raw rho: sigma = softplus(-5) = 0.0067
HBM_TBS = 6.3            # achievable HBM rate (tools/bench_metrics.py)
SEED = 11


class Clock:
    """Wall-clock milliseconds per part of a leg."""

    def __init__(self):
        self.ms = {}

    def time(self, part, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        self.ms[part] = self.ms.get(part, 0.0) + (time.perf_counter() - t0) * 1e3
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bbb_lanes.py needs the GPU"
    x, y = synth.mnist_like(N_ROWS * 5 // 4, seed=1234)                  # the training split (80 %) has N_ROWS rows
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
    cfg = sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS))
    hp = HyperParameters(**BASE)
    xv, yv = ds.valid_data.as_numpy()
    xv_dev = torch.as_tensor(np.ascontiguousarray(np.asarray(xv, dtype=np.float32).reshape(len(xv), -1))).cuda()
    yv = np.asarray(yv).reshape(-1).astype(np.int64)
    n_valid = len(yv)
    points = [(lr, al) for lr in LRS for al in ALPHAS]

    def lanes_leg():
        clock = Clock()
        obj = BBBGridObjective(hp, cfg, ds, args.steps, GaussianPrior(*PRIOR), metric="val_error", weights="mu", seed=SEED,
                               max_lanes=32)
        train, scores, compile_ = BBB.train, BBB.lane_scores, BBB.compile
        BBB.compile = lambda self, *a, **k: clock.time("compile", lambda: compile_(self, *a, **k))
        BBB.train = lambda self, *a, **k: clock.time("train", lambda: train(self, *a, **k))
        BBB.lane_scores = lambda self, *a, **k: clock.time("score", lambda: scores(self, *a, **k))
        try:
            grid = GridOptimizer()
            grid.compile(obj, Real(LRS[0], LRS[-1], "lr"), Real(ALPHAS[0], ALPHAS[-1], "alpha"), n=2,
                         specify={"lr": LRS, "alpha": ALPHAS}, verbose=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grid.optimize()
            total = (time.perf_counter() - t0) * 1e3
        finally:
            BBB.compile, BBB.train, BBB.lane_scores = compile_, train, scores
        assert obj.trainings == [32] and list(grid.results) == points
        return total, clock.ms, grid.results

    def serial_leg():
        clock = Clock()
        results = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for lr, al in points:
            opt = BBB()
            clock.time("compile", lambda: opt.compile(HyperParameters(**{**BASE, "lr": lr, "alpha": al}), cfg, ds, verbose=False,
                                                      seed=SEED, prior=GaussianPrior(*PRIOR)))
            clock.time("train", lambda: opt.train(args.steps))

            def score():
                w, B, wrong = opt._mu[None, :].contiguous(), opt._plan.max_batch, 0
                for r0 in range(0, n_valid, B):
                    _, mean = opt._plan.predict(w, xv_dev[r0:r0 + B], want_samples=False)
                    wrong += int((np.argmax(mean.cpu().numpy(), axis=1) != yv[r0:r0 + B]).sum())
                return wrong / n_valid
            results[(lr, al)] = clock.time("score", score)
            opt._plan.close()
            if getattr(opt, "_val_plan", None) is not None:
                opt._val_plan.close()
        return (time.perf_counter() - t0) * 1e3, clock.ms, results

    legs = {"lanes": lanes_leg, "serial": serial_leg}
    first = {k: fn() for k, fn in legs.items()}                          # warm-up of both legs (allocator, graph capture)
    rounds = {k: [] for k in legs}
    parts = {k: {} for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            total, ms, _ = fn()
            rounds[k].append(total)
            for part, t in ms.items():
                parts[k].setdefault(part, []).append(t)
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    out = {"tool": "bench_bbb_lanes", "shape": "784-400-400-10", "batch": BATCH, "ragged_batch": 896, "steps": args.steps,
           "points": len(points), "valid_rows": n_valid, "rounds": args.rounds}
    for k in legs:
        out[k] = {"ms": round(med[k], 2), "us_per_lane_step": round(med[k] * 1e3 / (len(points) * args.steps), 2),
                  "train_us_per_lane_step": round(float(np.median(parts[k]["train"])) * 1e3 / (len(points) * args.steps), 2),
                  "parts_ms": {part: round(float(np.median(v)), 2) for part, v in parts[k].items()}}
    out["serial_over_lanes_whole"] = round(med["serial"] / med["lanes"], 3)
    out["serial_over_lanes_train"] = round(out["serial"]["parts_ms"]["train"] / out["lanes"]["parts_ms"]["train"], 3)
    a = np.array([first["lanes"][2][p] for p in points])
    b = np.array([first["serial"][2][p] for p in points])
    out["scores"] = {"lanes_best": list(points[int(a.argmin())]), "serial_best": list(points[int(b.argmin())]),
                     "max_abs_diff": float(np.max(np.abs(a - b))), "lanes_min_max": [float(a.min()), float(a.max())]}

    # ---- the per-kernel split: 8 steps of the 32-lane step, 8 single steps beside it
    P = len(points)
    plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=BATCH, max_particles=P)
    D = plan.D
    xd, yd = torch.as_tensor(x[:N_ROWS].reshape(N_ROWS, -1)).cuda(), torch.as_tensor(y[:N_ROWS].astype(np.int32)).cuda()
    idx, sizes = synth.batch_plan(N_ROWS, BATCH, 16)
    idx_d = torch.as_tensor(idx).cuda()
    mu = torch.as_tensor(synth.glorot_uniform(DIMS)).cuda().repeat(P, 1).contiguous()
    rho, w = torch.full((P, D), PRIOR[1], device="cuda"), torch.zeros((P, D), device="cuda")
    cost = torch.zeros((P, 4), device="cuda")
    tabs = [np.array([p[0] for p in points], dtype=np.float32), np.array([p[1] for p in points], dtype=np.float32),
            np.full(P, PRIOR[0], dtype=np.float32), np.full(P, PRIOR[1], dtype=np.float32)]
    mu1, rho1, w1, cost1 = mu[0].clone(), rho[0].clone(), w[0].clone(), torch.zeros(4, device="cuda")

    def lanes_steps(n, first_step):
        for s in range(n):
            plan.bbb_lanes_step(mu, rho, w, xd, yd, *tabs, first_step + s, 7, cost, batch=sizes[s], row_idx=idx_d[s])

    def single_steps(n, first_step):
        for s in range(n):
            plan.bbb_step(mu1, rho1, w1, xd, yd, BASE["lr"], BASE["alpha"], PRIOR[0], PRIOR[1], first_step + s, 7, cost1,
                          batch=sizes[s], row_idx=idx_d[s])
    lanes_steps(2, 1)
    single_steps(2, 1)
    out["kernels"] = {}
    for tag, fn in (("lanes_step", lanes_steps), ("single_step", single_steps), ("lanes_step_again", lanes_steps),
                    ("single_step_again", single_steps)):
        with engine.KernelProbe(512) as kp:
            fn(8, 3)
        out["kernels"][tag] = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}
        out["kernels"][tag + "_us"] = round(sum(t for _, t in kp.launches) / 8, 2)
    by = out["kernels"]["lanes_step_again"]
    out["streaming"] = {}
    for name, floats in (("k_bbb_sample_lanes", 3), ("k_bbb_update_lanes", 6)):
        us = by[name][1]
        nbytes = 4 * floats * P * D
        out["streaming"][name] = {"us": us, "bytes": nbytes, "tb_per_s": round(nbytes / us * 1e-6, 4),
                                  "fraction_of_hbm": round(nbytes / us * 1e-6 / HBM_TBS, 4)}
    out["lanes_step_us_per_lane"] = round(out["kernels"]["lanes_step_again_us"] / P, 2)
    out["rounds_ms"] = {k: [round(t, 2) for t in v] for k, v in rounds.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
