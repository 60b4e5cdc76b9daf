#!/usr/bin/env python3
"""Per-step cost of BSAM at the C2 shape (GPU box): 784 -> 200 -> 10, batch 1024, 7 * 1024 + 896 synthetic MNIST-shaped
rows (synth.mnist_like), so every eighth batch is the ragged 896-row one -- the shape and batch table of
tools/bench_adam.py.  Each variant runs the same batch table through its eager per-step entry point:
    bsam           pyz_bsam_step                              (Philox noise; perturb + two gradient passes, 7 launches)
    sgd            pyz_sgd_step
    perturb_2sgd   pyz_vadam_perturb + 2 x pyz_sgd_step       (the same number of gradient passes, from entry points
                                                               that predate BSAM: the figure to judge `bsam` by)
us_per_step: device events around `--steps` steps (host enqueue included), median of `--rounds` rounds with the
variants alternating inside each round.  kernel_us_per_step: the sum of the kernels' own durations per step
(KernelProbe) over 16 steps, and `kernels` the split by kernel.
resident: the same steps as device-resident runs (tools/resident_legs.py), in us per step, every leg once per round in turn
-- `eager` (the loop above, measured again beside the others), `run` (the bare C-ABI run), `run_unfused`
(PYZ_ADAM_FUSE_PERTURB=0, a child process), `train_run` (a quiet train() through the run) and `train_loop` (the same call
with PYZ_ADAM_RUN=0); `resident_rounds` keeps every round.  Prints one JSON line."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bayesian_inference_for_nn_amd import engine, synth  # noqa: E402

import resident_legs  # noqa: E402  (tools/ is the script's directory)

DIMS, ACTS = (784, 200, 10), ("relu", "softmax")
BATCH, N_ROWS = 1024, 7 * 1024 + 896
# a learning rate and sharpness at which 400 steps from Glorot weights stay finite; the cost does not depend on them
LR, BETA_1, BETA_2, LAM, RHO, GAM = 1e-3, 0.9, 0.999, 0.5, 1e-3, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bsam.py needs the GPU"
    x, y = synth.mnist_like(N_ROWS, seed=1234)
    xd, yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    n_tab = max(args.steps, args.warmup, 16)
    idx, sizes = synth.batch_plan(N_ROWS, BATCH, n_tab)
    assert 896 in sizes
    idx_d = torch.as_tensor(idx).cuda()
    plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=BATCH)
    D = plan.D
    theta0 = torch.as_tensor(synth.glorot_uniform(DIMS)).cuda()
    kinds = ("bsam", "sgd", "perturb_2sgd")
    state = {k: (theta0.clone(), torch.zeros(D, device="cuda"), torch.ones(D, device="cuda")) for k in kinds}
    loss = torch.zeros(2, device="cuda")
    loss1 = loss[:1]
    count = {"bsam": 0, "perturb_2sgd": 0}

    def step(kind, s):
        th, m, v = state[kind]
        b, rows = sizes[s], idx_d[s]
        if kind == "bsam":
            plan.bsam_step(th, m, v, xd, yd, LR, BETA_1, BETA_2, LAM, RHO, GAM, float(N_ROWS), count[kind], 7, loss, batch=b,
                           row_idx=rows)
            count[kind] += 1
        elif kind == "sgd":
            plan.sgd_step(th, xd, yd, LR, loss1, batch=b, row_idx=rows)
        else:
            plan.vadam_perturb(th, v, LAM, float(N_ROWS), count[kind], 7)
            count[kind] += 1
            plan.sgd_step(th, xd, yd, LR, loss1, batch=b, row_idx=rows)
            plan.sgd_step(th, xd, yd, LR, loss1, batch=b, row_idx=rows)

    for k in kinds:
        for s in range(args.warmup):
            step(k, s)
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k in kinds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in range(args.steps):
                step(k, s)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    us = {k: float(np.median(v)) for k, v in times.items()}

    def eager_round(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(args.steps):
            step(k, s)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps

    res_kinds = ("bsam",)
    res_times = resident_legs.measure(res_kinds, args.steps, 1, args.rounds, {k: (lambda k=k: eager_round(k)) for k in res_kinds})
    kernel_us, split = {}, {}
    for k in kinds:
        with engine.KernelProbe(256) as kp:
            for s in range(16):
                step(k, s)
        kernel_us[k] = sum(t for _, t in kp.launches) / 16
        split[k] = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}
    plan.check_finite()
    print(json.dumps({"tool": "bench_bsam", "shape": "784-200-10", "batch": BATCH, "ragged_batch": 896, "steps": args.steps,
                      "rounds": args.rounds, "us_per_step": {k: round(v, 2) for k, v in us.items()},
                      "us_per_step_rounds": {k: [round(t, 2) for t in v] for k, v in times.items()},
                      "ratio_bsam_perturb_2sgd": round(us["bsam"] / us["perturb_2sgd"], 3),
                      "ratio_bsam_sgd": round(us["bsam"] / us["sgd"], 3),
                      "kernel_us_per_step": {k: round(v, 2) for k, v in kernel_us.items()},
                      "kernel_ratio_bsam_perturb_2sgd": round(kernel_us["bsam"] / kernel_us["perturb_2sgd"], 3),
                      "kernels": split,
                      "resident": resident_legs.summary(res_times), "resident_rounds": res_times}))


if __name__ == "__main__":
    main()
