#!/usr/bin/env python3
"""Cost of SGLD with P chains per launch against P single-chain runs back to back, at the C2 shape (GPU box):
784 -> 200 -> 10, batch 1024, 7 * 1024 + 896 synthetic MNIST-shaped rows (synth.mnist_like), so every eighth batch is the
ragged 896-row one.  For P in --chains (default 1 2 4 8 16 32), in us per step and per chain-step (= per step / P):
    step_loop    `--steps` calls of pyz_sgld_chains_step (device events around the loop, host enqueue included)
    run          pyz_sgld_chains_run over the same batch table
    train        a quiet SGLD.train(--steps) of an optimizer compiled with n_chains = P (wall clock: it joins its run)
    kernels      {kernel: [launches, mean us]} of 8 steps under KernelProbe, and kernel_us_per_step, their sum per step
    update       k_sgld_update_chains alone: mean us, the bytes it moves (7 floats per element: theta, mean and sq_mean read
                 and written, the gradient read), bytes / s and the fraction of the 6.3 TB/s achievable HBM rate
baseline: single-chain pyz_sgld_run (hipGraph replay; the code path n_chains does not touch) in the same process, the
same way: us per step = us per chain-step.  chain_steps_per_s compares the legs; `speedup_run_vs_baseline` = baseline us per
chain-step / the run's.  Every leg is measured once per round, the legs in turn inside a round; the figures are medians of
--rounds rounds and `rounds` keeps every round.  Prints one JSON line."""

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

DIMS, ACTS = (784, 200, 10), ("relu", "softmax")
BATCH, N_ROWS = 1024, 7 * 1024 + 896
LR_UPPER, LR_LOWER, LR_GAMMA = 0.01, 0.003, 0.99
HBM_TBS = 6.3            # achievable HBM rate (tools/bench_metrics.py)
UPDATE = "k_sgld_update_chains"


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def quiet_optimizer(P, steps):
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
    from bayesian_inference_for_nn_amd.nn import sequential_json
    from bayesian_inference_for_nn_amd.optimizers import SGLD
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    x, y = synth.mnist_like(N_ROWS * 5 // 4, seed=1234)                  # the training split (80 %) has N_ROWS rows
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
    opt = SGLD()
    kw = {"n_chains": P} if P > 1 else {}
    opt.compile(HyperParameters(lr_upper=LR_UPPER, lr_lower=LR_LOWER, lr_gamma=LR_GAMMA, batch_size=BATCH),
                sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS)), ds, verbose=False, seed=11, **kw)
    opt.train(steps)                                                    # warm-up: buffers, tables
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chains", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--no-train", action="store_true", help="skip the SGLD.train leg")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sgld_chains.py needs the GPU"
    x, y = synth.mnist_like(N_ROWS, seed=1234)
    xd, yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    n_tab = max(args.steps, args.warmup, 16)
    idx, sizes = synth.batch_plan(N_ROWS, BATCH, n_tab)
    assert 896 in sizes
    idx_d = torch.as_tensor(idx).cuda()
    lrs = synth.sgld_lr_table(n_tab, LR_UPPER, LR_LOWER, LR_GAMMA, 0, n_tab).tolist()
    stream = torch.cuda.Stream()
    out = {"tool": "bench_sgld_chains", "shape": "784-200-10", "batch": BATCH, "ragged_batch": 896, "steps": args.steps,
           "rounds": args.rounds, "chains": {}}

    # ---- the baseline: single-chain pyz_sgld_run
    base_plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=BATCH)
    D = base_plan.D
    theta0 = torch.as_tensor(synth.glorot_uniform(DIMS)).cuda()
    b_state = (theta0.clone(), torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"))
    b_losses = torch.zeros(n_tab, device="cuda")

    def baseline():
        with torch.cuda.stream(stream):
            return events(lambda: base_plan.sgld_run(*b_state, xd, yd, idx_d, sizes[:args.steps], lrs[:args.steps], 0, 7,
                                                     b_losses, use_graph=True)) / args.steps

    legs = {"baseline": baseline}
    plans, opts = {}, {}
    for P in args.chains:
        plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=BATCH, max_particles=P)
        st = (theta0.repeat(P, 1).contiguous(), torch.zeros((P, D), device="cuda"), torch.zeros((P, D), device="cuda"))
        loss = torch.zeros(P, device="cuda")
        losses = torch.zeros((n_tab, P), device="cuda")
        plans[P] = (plan, st, loss, losses)

        def step_loop(plan=plan, st=st, loss=loss):
            def body():
                for s in range(args.steps):
                    plan.sgld_chains_step(*st, xd, yd, lrs[s], s, 7, loss, batch=sizes[s], row_idx=idx_d[s])
            return events(body) / args.steps

        def run(plan=plan, st=st, losses=losses):
            with torch.cuda.stream(stream):
                return events(lambda: plan.sgld_chains_run(*st, xd, yd, idx_d, sizes[:args.steps], lrs[:args.steps], 0, 7,
                                                           losses)) / args.steps
        legs[f"step_loop_p{P}"] = step_loop
        legs[f"run_p{P}"] = run
        if not args.no_train:
            opts[P] = quiet_optimizer(P, args.steps)

            def train(opt=opts[P]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                opt.train(args.steps)
                return (time.perf_counter() - t0) * 1e6 / args.steps
            legs[f"train_p{P}"] = train

    for fn in legs.values():                                             # warm-up of every leg (graph capture, tables)
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            rounds[k].append(fn())
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    out["baseline"] = {"entry": "pyz_sgld_run", "us_per_step": round(med["baseline"], 2),
                       "chain_steps_per_s": round(1e6 / med["baseline"], 1), "path": base_plan.last_run_path()[0]}
    for P in args.chains:
        plan, st, loss, losses = plans[P]
        with engine.KernelProbe(256) as kp:
            for s in range(8):
                plan.sgld_chains_step(*st, xd, yd, lrs[s], s, 7, loss, batch=sizes[s], row_idx=idx_d[s])
        by = kp.by_kernel()
        upd_us = by[UPDATE][1]
        nbytes = 7 * 4 * P * D
        entry = {"kernels": {name: [c, round(t, 2)] for name, (c, t) in by.items()},
                 "kernel_us_per_step": round(sum(t for _, t in kp.launches) / 8, 2),
                 "update": {"us": round(upd_us, 2), "bytes": nbytes, "tb_per_s": round(nbytes / upd_us * 1e-6, 3),
                            "fraction_of_hbm": round(nbytes / upd_us * 1e-6 / HBM_TBS, 3)}}
        for leg in ("step_loop", "run", "train"):
            k = f"{leg}_p{P}"
            if k in med:
                entry[leg] = {"us_per_step": round(med[k], 2), "us_per_chain_step": round(med[k] / P, 2),
                              "chain_steps_per_s": round(P * 1e6 / med[k], 1)}
        entry["speedup_run_vs_baseline"] = round(med["baseline"] / (med[f"run_p{P}"] / P), 3)
        try:
            plan.check_finite()
        except Exception as e:                                           # a diverged chain does not void the timing: say so
            entry["nonfinite"] = str(e)
        out["chains"][str(P)] = entry
    out["rounds_us_per_step"] = {k: [round(t, 2) for t in v] for k, v in rounds.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
