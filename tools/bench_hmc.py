#!/usr/bin/env python3
"""Per-proposal cost of HMC at the C3 shape of BASELINE.md (GPU box): make_moons(2000) -> 1600 training rows, 2 -> 50 -> 2,
L = 20, epsilon = 0.005, m = 0.5, prior (0, 1), for 1 and 8 chains.  Four figures per chain count:
    train_run     HMC.train(verbose off) through pyz_hmc_run (one device-resident run, one join)
    train_loop    the same call with PYZ_HMC_RUN=0 (the step loop: one pyz_hmc_step and two snapshot kernels per proposal)
    cabi_loop     a loop of pyz_hmc_step on a side stream, nothing else
    kernel        the sum of the kernels' own durations per proposal (KernelProbe over 16 pyz_hmc_step calls), and the split
                  (`kernels`: {kernel: [launches per proposal, mean us per launch]})
us per proposal: a host clock around work that ends in a join (train_*: the 10 burn-in proposals count as proposals) or
device events around the loop (cabi_loop), `--steps` proposals per window, median of `--rounds` rounds with the
variants alternating inside each round; `spread` is (max - min) / median over the rounds of a variant.  Prints one JSON
line."""

import argparse
import json
import os
import random
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
from bayesian_inference_for_nn_amd.optimizers import HMC  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters  # noqa: E402

DIMS, ACTS = (2, 50, 2), ("relu", "softmax")
L, EPS, MASS = 20, 0.005, 0.5
BURN = 10


def optimizer(ds, chains):
    opt = HMC()
    opt.compile(HyperParameters(epsilon=EPS, m=MASS, L=L), sequential_json(2, [50, 2], list(ACTS)), ds, verbose=False,
                prior=GaussianPrior(0.0, 1.0), seed=7, n_chains=chains)
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chains", type=int, nargs="+", default=[1, 8])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hmc.py needs the GPU"
    assert args.steps > BURN
    x, y = synth.moons(2000, seed=42)
    out = {"tool": "bench_hmc", "shape": "2-50-2", "rows": 1600, "L": L, "steps": args.steps, "rounds": args.rounds, "chains": {}}
    for chains in args.chains:
        ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=3)
        opts = {"train_run": optimizer(ds, chains), "train_loop": optimizer(ds, chains)}
        assert opts["train_run"]._batch_size == 1600
        # the bare loop: its own plan, buffers and stream
        plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=1600, max_particles=chains)
        src = opts["train_run"]
        xd, yd = src._x_dev, src._y_dev
        q, stats = torch.zeros((chains, plan.D), device="cuda"), torch.zeros((chains, 8), device="cuda")
        side = torch.cuda.Stream()
        us = [0.5] * chains
        count = [0]

        def cabi(n):
            with torch.cuda.stream(side):
                for _ in range(n):
                    plan.hmc_step(q, xd, yd, L, EPS, MASS, 0.0, 1.0, us, count[0], 7, stats)
                    count[0] += 1

        def train(kind, n):
            os.environ["PYZ_HMC_RUN"] = "1" if kind == "train_run" else "0"
            opts[kind].train(n - BURN)

        random.seed(1)
        for kind in opts:                      # warm-up at the timed length: the graphs of that length are captured here
            train(kind, args.warmup)
            train(kind, args.steps)
        cabi(args.warmup)
        torch.cuda.synchronize()
        assert opts["train_run"]._plan.last_run_path()[1] == args.steps, "train_run did not take pyz_hmc_run"
        assert opts["train_loop"]._plan.last_run_path()[1] == 0
        times = {"train_run": [], "train_loop": [], "cabi_loop": []}
        for _ in range(args.rounds):
            for kind in times:
                torch.cuda.synchronize()
                if kind == "cabi_loop":
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(side):
                        e0.record()
                    cabi(args.steps)
                    with torch.cuda.stream(side):
                        e1.record()
                    e1.synchronize()
                    times[kind].append(e0.elapsed_time(e1) * 1e3 / args.steps)
                else:
                    t0 = time.perf_counter()
                    train(kind, args.steps)
                    torch.cuda.synchronize()
                    times[kind].append((time.perf_counter() - t0) * 1e6 / args.steps)
        torch.cuda.synchronize()
        with engine.KernelProbe(1024) as kp:       # (on the default stream: a side stream replays the proposal's graph, which the probe does not see)
            for _ in range(16):
                plan.hmc_step(q, xd, yd, L, EPS, MASS, 0.0, 1.0, us, count[0], 7, stats)
                count[0] += 1
        assert kp.launches, "the probe saw no launch"
        med = {k: float(np.median(v)) for k, v in times.items()}
        out["chains"][str(chains)] = {
            "us_per_proposal": {k: round(v, 2) for k, v in med.items()},
            "rounds_us": {k: [round(t, 2) for t in v] for k, v in times.items()},
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()},
            "ratio_run_over_loop": round(med["train_run"] / med["train_loop"], 4),
            "kernel_us_per_proposal": round(sum(t for _, t in kp.launches) / 16, 2),
            "kernels": {name: [round(c / 16, 3), round(t, 2)] for name, (c, t) in kp.by_kernel().items()},
            "run_path": list(opts["train_run"]._plan.last_run_path()),
            "accept_rate_run": round(opts["train_run"]._accepted_runs / max(opts["train_run"]._total_runs, 1), 3),
        }
        plan.close()
    os.environ.pop("PYZ_HMC_RUN", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
