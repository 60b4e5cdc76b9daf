#!/usr/bin/env python3
"""Cost of one FSVI step (GPU box): MLPPlan.fsvi_step on seeded data, default the 1 -> 50 -> 1 model (D = 151), k = 10
particles, batch_size = 128 (n = 256 rows per particle), draws from the device's Philox stream.
    step_ms      ms per step: --steps steps after --warmup ones, host clock around calls that end in a stream synchronise,
                 the median of --rounds rounds
    kernels      {kernel: [launches, mean us]} of one step (KernelProbe: each launch's own begin / end timestamps) and
                 their sum; gp_solve_us / stein_solve_us tell the two k_spd_solve_f64 launches of a step apart
    workspace_mib  the plan's workspace after the first step (the two float64 systems included)
Prints one JSON line.  --trace-only runs the steps and prints nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --`, in a run of its own."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPPlan, MLPSpec  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fsvi needs the GPU: a CPU run says nothing about it")
    rng = np.random.default_rng(0)
    k, B = a.k, a.batch_size
    spec = MLPSpec((1, a.hidden, 1), ("relu", "linear"), "mse")
    x = rng.uniform(-3, 3, size=(4 * B, 1)).astype(np.float32)
    y = (2 * x + 2).astype(np.float32)
    plan = MLPPlan(spec, max_batch=2 * B, max_particles=k)
    D = plan.D
    xd, yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    lo, hi = xd.min(dim=0).values.contiguous(), xd.max(dim=0).values.contiguous()
    mu = torch.zeros(D, device="cuda")
    W = torch.as_tensor(rng.normal(size=(k, D)).astype(np.float32)).cuda()
    m, v, loss = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros(1, device="cuda")
    idx = torch.as_tensor(rng.permutation(len(x))[:B].astype(np.int32)).cuda()
    t = 0

    def step():
        nonlocal t
        t += 1
        plan.fsvi_step(mu, W, m, v, xd, yd, B, 1e-3, t, 7, loss, lo=lo, hi=hi, batch=B, row_idx=idx)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    if a.trace_only:
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        return
    ms = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
    with KernelProbe(64) as kp:
        step()
    plan.check_finite()
    solves = [us for name, us in kp.launches if name.startswith("k_spd_solve_f64")]   # launch order: Stein, then GP
    out = {"tool": "bench_fsvi", "model": list(spec.dims), "D": D, "k": k, "batch_size": B, "n": 2 * B, "steps": a.steps,
           "warmup": a.warmup, "step_ms": float(np.median(ms)), "ms_rounds": ms,
           "kernels": {name: [c, round(us, 2)] for name, (c, us) in sorted(kp.by_kernel().items())},
           "stein_solve_us": round(solves[0], 2), "gp_solve_us": round(solves[1], 2),
           "kernel_us_total": round(sum(us for _, us in kp.launches), 1), "launches": len(kp.launches),
           "workspace_mib": round(plan.workspace_bytes / 2 ** 20, 2), "loss": float(loss.item())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
