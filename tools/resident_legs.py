#!/usr/bin/env python3
"""The device-resident legs of tools/bench_adam.py and tools/bench_bsam.py at the C2 shape (784 -> 200 -> 10, batch 1024,
7 * 1024 + 896 rows: every eighth batch is the ragged one), in us per step:
    train_run    a quiet <class>.train(steps): pyz_adam_run / pyz_bsam_run in resident chunks (wall clock, train() joins)
    train_loop   the same call with PYZ_ADAM_RUN=0: the per-step loop of Optimizer.train
    run          the bare C-ABI run, one call of `steps` steps (device events, host enqueue included)
    run_unfused  ... with PYZ_ADAM_FUSE_PERTURB=0.  The library reads that switch once, so this leg lives in a child
                 process that the parent asks for one round at a time: its rounds alternate with the others'.
The callers add their eager C-ABI loop and alternate all legs inside each round."""

import os
import select
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS, ACTS = (784, 200, 10), ("relu", "softmax")
BATCH, N_ROWS = 1024, 7 * 1024 + 896
HYP = {
    "adam": dict(lr=1e-3, beta_1=0.9, beta_2=0.999, batch_size=BATCH),
    "vadam": dict(lr=1e-3, beta_1=0.9, beta_2=0.999, batch_size=BATCH, lam=0.5),
    "bsam": dict(lr=1e-3, beta_1=0.9, beta_2=0.999, batch_size=BATCH, lam=0.5, rho=1e-3, gam=0.1),
}


class BareRun:
    """`steps` steps of one kind through the run entry point, on persistent buffers (the graphs are captured once)."""

    def __init__(self, kind, steps):
        import torch
        from bayesian_inference_for_nn_amd import engine, synth
        self.kind, self.steps, self.torch = kind, steps, torch
        x, y = synth.mnist_like(N_ROWS, seed=1234)
        self.xd, self.yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
        idx, self.sizes = synth.batch_plan(N_ROWS, BATCH, steps)
        self.idx = torch.as_tensor(idx).cuda()
        self.plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=BATCH)
        D = self.plan.D
        self.theta0 = torch.as_tensor(synth.glorot_uniform(DIMS)).cuda()
        self.th, self.m = self.theta0.clone(), torch.zeros(D, device="cuda")
        self.v = (torch.ones if kind == "bsam" else torch.zeros)(D, device="cuda")
        self.losses = torch.zeros(2 * steps, device="cuda")
        self.stream = torch.cuda.Stream()
        self.step0 = 0

    def __call__(self):
        torch, h, n = self.torch, HYP[self.kind], self.steps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            e0.record()
            if self.kind == "bsam":
                self.plan.bsam_run(self.th, self.m, self.v, self.xd, self.yd, self.idx, self.sizes, [h["lr"]] * n, h["beta_1"],
                                   h["beta_2"], h["lam"], h["rho"], h["gam"], float(N_ROWS), self.step0, 7, self.losses)
            else:
                vd = self.kind == "vadam"
                lam_n = 0.5 / N_ROWS
                self.plan.adam_run(self.th, self.m, self.v, self.xd, self.yd, self.idx, self.sizes, [h["lr"]] * n,
                                   [1 + s // 8 for s in range(n)], h["beta_1"], h["beta_2"], self.losses,
                                   denom_eps=lam_n if vd else 1e-3, decay=lam_n if vd else 0.0, perturb=vd, lam=0.5,
                                   num_data=float(N_ROWS), step0=self.step0, seed=7)
            e1.record()
        e1.synchronize()
        self.step0 += n
        return e0.elapsed_time(e1) * 1e3 / n


class Trainer:
    """A compiled optimizer of the kind on N_ROWS training rows; train(steps) through the run or the step loop."""

    def __init__(self, kind, steps):
        import torch
        from bayesian_inference_for_nn_amd import synth
        from bayesian_inference_for_nn_amd.datasets import Dataset
        from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
        from bayesian_inference_for_nn_amd.nn import model_from_json, sequential_json
        from bayesian_inference_for_nn_amd.optimizers import ADAM, BSAM, VADAM
        from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
        self.steps, self.torch = steps, torch
        x, y = synth.mnist_like(N_ROWS * 5 // 4, seed=1234)              # the training split is 80 %
        ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
        assert ds.train_size == N_ROWS, ds.train_size
        cfg = sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS))
        start = model_from_json(cfg)
        start.reset_glorot(np.random.default_rng(9))
        self.opt = {"adam": ADAM, "vadam": VADAM, "bsam": BSAM}[kind]()
        self.opt.compile(HyperParameters(**HYP[kind]), cfg, ds, verbose=False, starting_model=start, seed=11)

    def __call__(self, resident=True):
        old = os.environ.get("PYZ_ADAM_RUN")
        os.environ["PYZ_ADAM_RUN"] = "1" if resident else "0"
        try:
            self.torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.opt.train(self.steps)
            self.torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / self.steps
        finally:
            if old is None:
                os.environ.pop("PYZ_ADAM_RUN", None)
            else:
                os.environ["PYZ_ADAM_RUN"] = old


class UnfusedChild:
    """The bare run in a child process started with PYZ_ADAM_FUSE_PERTURB=0; one round per request."""

    ROUND_LIMIT_S = 120          # the first round builds the plan and captures the graphs; a round itself takes milliseconds

    def __init__(self, kind, steps):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), kind, str(steps)], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=dict(os.environ, PYZ_ADAM_FUSE_PERTURB="0"))

    def __call__(self):
        self.p.stdin.write("round\n")
        self.p.stdin.flush()
        ready, _, _ = select.select([self.p.stdout], [], [], self.ROUND_LIMIT_S)
        if not ready:
            self.p.kill()
            raise RuntimeError(f"the unfused child gave no answer within {self.ROUND_LIMIT_S} s")
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"the unfused child ended (exit status {self.p.wait()})")
        return float(line)

    def close(self):
        self.p.stdin.close()
        try:
            return self.p.wait(timeout=60)
        except subprocess.TimeoutExpired:
            self.p.kill()
            return self.p.wait()


def measure(kinds, steps, warmup_rounds, rounds, eager):
    """eager: {kind: callable() -> us per step of the eager C-ABI loop}.  Returns {kind: {leg: [us per round]}} with
    every leg of every kind taken once per round, in turn."""
    legs = {}
    for k in kinds:
        run, tr = BareRun(k, steps), Trainer(k, steps)
        legs[k] = {"eager": eager[k], "run": run, "train_run": tr, "train_loop": lambda tr=tr: tr(resident=False)}
        if k != "adam":
            legs[k]["run_unfused"] = UnfusedChild(k, steps)
    times = {k: {leg: [] for leg in legs[k]} for k in kinds}
    try:
        for r in range(warmup_rounds + rounds):
            for k in kinds:
                for leg, fn in legs[k].items():
                    us = fn()
                    if r >= warmup_rounds:
                        times[k][leg].append(round(us, 2))
    finally:
        for k in kinds:
            if "run_unfused" in legs[k]:
                legs[k]["run_unfused"].close()
    return times


def summary(times):
    return {k: {leg: round(float(np.median(v)), 2) for leg, v in t.items()} for k, t in times.items()}


def child_main(kind, steps):
    run = BareRun(kind, steps)
    for line in sys.stdin:
        if line.strip() != "round":
            break
        print(run(), flush=True)
    run.plan.check_finite()


if __name__ == "__main__":
    child_main(sys.argv[1], int(sys.argv[2]))
