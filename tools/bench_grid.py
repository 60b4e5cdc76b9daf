#!/usr/bin/env python3
"""Cost of a hyper-parameter grid search on SGLD lanes against the same grid point by point, at the C2 shape (GPU box):
784 -> 200 -> 10, batch 1024, synthetic MNIST-shaped rows (synth.mnist_like) with 7 * 1024 + 896 rows in the training split,
so every eighth batch is the ragged 896-row one.  The grid: 8 values of lr_upper x 4 of lr_gamma = 32 points, --steps
(default 200) SGLD steps each, scored by the mean loss on the validation split.
    lanes    GridOptimizer + SGLDGridObjective(max_lanes=32): ONE SGLD compiled with 32 lanes, one quiet train (pyz_sgld_lanes_run),
             one lane_scores (pyz_lane_scores) -- the scores never leave the device before they are 32 numbers
    serial   the reference's loop: per point an SGLD compiled with the point's hyper-parameters, a quiet single-chain train
             (pyz_sgld_run), the validation split through plan.predict, the (rows, 10) probabilities to the host and the loss
             there
Both legs start every training from the same seed.  The legs alternate inside one process; each is timed as a whole (wall
clock, it ends with its scores on the host) and split into compile / train / score; the figures are medians of --rounds
rounds and `rounds_ms` keeps every round.  `kernels`: {kernel: [launches, mean us]} of 8 steps of the 32-lane step, of 8
steps of the 32-chain step beside it (k_sgld_update_chains against k_sgld_update_lanes in one process), of the lanes step once
more (`step_again`: a process's kernels get faster over its first launches) and of one lane_scores call under KernelProbe;
`lane_scores`: k_lane_scores alone, the bytes it reads (the lanes' logits and the labels once per lane), bytes / s and the
fraction of the 6.3 TB/s achievable HBM rate.  Prints one JSON line."""

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
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy  # noqa: E402
from bayesian_inference_for_nn_amd.nn import sequential_json  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers import SGLD  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import GridOptimizer, HyperParameters, Real, SGLDGridObjective  # noqa: E402

DIMS, ACTS = (784, 200, 10), ("relu", "softmax")
BATCH, N_ROWS = 1024, 7 * 1024 + 896
BASE = dict(lr_upper=0.01, lr_lower=0.003, lr_gamma=0.99, batch_size=BATCH)
UPPER = [0.004 + 0.002 * i for i in range(8)]
GAMMA = [0.6, 0.75, 0.9, 0.99]
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
    assert torch.cuda.is_available(), "bench_grid.py needs the GPU"
    x, y = synth.mnist_like(N_ROWS * 5 // 4, seed=1234)                  # the training split (80 %) has N_ROWS rows
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
    cfg = sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS))
    hp = HyperParameters(**BASE)
    xv, yv = ds.valid_data.as_numpy()
    xv_dev = torch.as_tensor(np.ascontiguousarray(np.asarray(xv, dtype=np.float32).reshape(len(xv), -1))).cuda()
    yv = np.asarray(yv).reshape(-1).astype(np.int64)
    n_valid = len(yv)
    points = [(u, g) for u in UPPER for g in GAMMA]

    def lanes_leg():
        clock = Clock()
        obj = SGLDGridObjective(hp, cfg, ds, args.steps, metric="val_loss", seed=SEED, max_lanes=32)
        # the parts of the one training, timed where the objective calls them
        train, scores, compile_ = SGLD.train, SGLD.lane_scores, SGLD.compile
        SGLD.compile = lambda self, *a, **k: clock.time("compile", lambda: compile_(self, *a, **k))
        SGLD.train = lambda self, *a, **k: clock.time("train", lambda: train(self, *a, **k))
        SGLD.lane_scores = lambda self, *a, **k: clock.time("score", lambda: scores(self, *a, **k))
        try:
            grid = GridOptimizer()
            grid.compile(obj, Real(UPPER[0], UPPER[-1], "lr_upper"), Real(GAMMA[0], GAMMA[-1], "lr_gamma"), n=2,
                         specify={"lr_upper": UPPER, "lr_gamma": GAMMA}, verbose=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grid.optimize()
            total = (time.perf_counter() - t0) * 1e3
        finally:
            SGLD.compile, SGLD.train, SGLD.lane_scores = compile_, train, scores
        assert obj.trainings == [32] and list(grid.results) == points
        return total, clock.ms, grid.results

    def serial_leg():
        clock = Clock()
        results = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for u, g in points:
            opt = SGLD()
            clock.time("compile", lambda: opt.compile(HyperParameters(**{**BASE, "lr_upper": u, "lr_gamma": g}), cfg, ds,
                                                      verbose=False, seed=SEED))
            clock.time("train", lambda: opt.train(args.steps))

            def score():
                w, B, loss = opt._theta[None, :].contiguous(), opt._plan.max_batch, 0.0
                for r0 in range(0, n_valid, B):
                    _, mean = opt._plan.predict(w, xv_dev[r0:r0 + B], want_samples=False)
                    p = mean.cpu().numpy().astype(np.float64)
                    loss += float(-np.log(p[np.arange(len(p)), yv[r0:r0 + B]]).sum())
                return loss / n_valid
            results[(u, g)] = clock.time("score", score)
            opt._plan.close()
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
    out = {"tool": "bench_grid", "shape": "784-200-10", "batch": BATCH, "ragged_batch": 896, "steps": args.steps,
           "points": len(points), "valid_rows": n_valid, "rounds": args.rounds}
    for k in legs:
        out[k] = {"ms": round(med[k], 2), "us_per_point_step": round(med[k] * 1e3 / (len(points) * args.steps), 2),
                  "parts_ms": {part: round(float(np.median(v)), 2) for part, v in parts[k].items()}}
    out["speedup_whole"] = round(med["serial"] / med["lanes"], 3)
    out["speedup_train"] = round(out["serial"]["parts_ms"]["train"] / out["lanes"]["parts_ms"]["train"], 3)
    # the two legs rank the grid alike?  (the serial leg draws the noise of its one seed too; its gradients come from the
    # fused single-chain step, so the scores agree closely, not bit for bit)
    a = np.array([first["lanes"][2][p] for p in points])
    b = np.array([first["serial"][2][p] for p in points])
    out["scores"] = {"lanes_best": list(points[int(a.argmin())]), "serial_best": list(points[int(b.argmin())]),
                     "max_rel_diff": float(np.max(np.abs(a - b) / np.abs(b)))}

    # ---- the per-kernel split: 8 steps of the 32-lane step, one lane_scores call
    P = len(points)
    plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=BATCH, max_particles=P)
    D = plan.D
    xd, yd = torch.as_tensor(x[:N_ROWS].reshape(N_ROWS, -1)).cuda(), torch.as_tensor(y[:N_ROWS].astype(np.int32)).cuda()
    idx, sizes = synth.batch_plan(N_ROWS, BATCH, 16)
    idx_d = torch.as_tensor(idx).cuda()
    st = (torch.as_tensor(synth.glorot_uniform(DIMS)).cuda().repeat(P, 1).contiguous(), torch.zeros((P, D), device="cuda"),
          torch.zeros((P, D), device="cuda"))
    loss = torch.zeros(P, device="cuda")
    rates = np.full(P, 0.01, dtype=np.float32)
    n_sc = min(BATCH, n_valid)
    xs, ys = xv_dev[:n_sc].contiguous(), torch.as_tensor(yv[:n_sc].astype(np.int32)).cuda()
    for s in range(2):
        plan.sgld_lanes_step(*st, xd, yd, rates, s, 7, loss, batch=sizes[s], row_idx=idx_d[s])
    plan.lane_scores(st[0], xs, ys)
    with engine.KernelProbe(256) as kp:
        for s in range(8):
            plan.sgld_lanes_step(*st, xd, yd, rates, s, 7, loss, batch=sizes[s], row_idx=idx_d[s])
    by = kp.by_kernel()
    out["kernels"] = {"step": {name: [c, round(t, 2)] for name, (c, t) in by.items()},
                      "step_kernel_us": round(sum(t for _, t in kp.launches) / 8, 2)}
    # ... and, for the update kernel alone, the chains step of the same 32 rows in the same process
    plan.sgld_chains_step(*st, xd, yd, 0.01, 0, 7, loss, batch=sizes[0], row_idx=idx_d[0])
    with engine.KernelProbe(256) as kp:
        for s in range(8):
            plan.sgld_chains_step(*st, xd, yd, 0.01, s, 7, loss, batch=sizes[s], row_idx=idx_d[s])
    out["kernels"]["chains_step"] = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}
    with engine.KernelProbe(256) as kp:                                  # (and the lanes step once more: the order is not it)
        for s in range(8):
            plan.sgld_lanes_step(*st, xd, yd, rates, s, 7, loss, batch=sizes[s], row_idx=idx_d[s])
    out["kernels"]["step_again"] = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}
    with engine.KernelProbe(64) as kp:
        plan.lane_scores(st[0], xs, ys)
    by = kp.by_kernel()
    out["kernels"]["lane_scores"] = {name: [c, round(t, 2)] for name, (c, t) in by.items()}
    us = by["k_lane_scores"][1]
    nbytes = 4 * P * n_sc * DIMS[-1] + 4 * P * n_sc
    out["lane_scores"] = {"rows": n_sc, "lanes": P, "us": round(us, 2), "bytes": nbytes, "tb_per_s": round(nbytes / us * 1e-6, 4),
                          "fraction_of_hbm": round(nbytes / us * 1e-6 / HBM_TBS, 4)}
    out["rounds_ms"] = {k: [round(t, 2) for t in v] for k, v in rounds.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
