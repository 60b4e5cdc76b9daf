#!/usr/bin/env python3
"""Cost of SGD / SWAG with P members per launch against P single-model runs back to back, at the C2 shape (GPU box):
784 -> 200 -> 10, batch 1024, 7 * 1024 + 896 synthetic MNIST-shaped rows (synth.mnist_like), so every eighth batch is the
ragged 896-row one.  For each mode (swag, sgd) and P in --members (default 1 2 4 8 16 32), in us per step and per
member-step (= per step / P):
    step_loop    `--steps` calls of pyz_*_members_step (device events around the loop, host enqueue included)
    run          pyz_*_members_run over the same batch table
    train        a quiet train(--steps) of an optimizer compiled with n_members = P (wall clock: it joins its run)
    kernels      {kernel: [launches, mean us]} of 8 steps under KernelProbe, and kernel_us_per_step, their sum per step
    update       k_members_update alone on 8 steps of one kind: SWAG hit steps (8 floats per element: theta, mean and
                 sq_mean read and written, the gradient read, the deviation written) and SGD miss steps (3 floats: theta
                 read and written, the gradient read): mean us, bytes, bytes / s, the fraction of the 6.3 TB/s HBM rate
baseline: the single-model pyz_swag_run / pyz_sgd_run (hipGraph replay; the code path n_members does not touch) in the
same process, the same way.  `speedup_run_vs_baseline` = baseline us per step / the run's us per member-step.  Every leg
is measured once per round, the legs in turn inside a round; the figures are medians of --rounds rounds and
`rounds_us_per_step` keeps every round.  frequency = 5, k = 10 (the values the reference's SWAG scripts use).  Prints one
JSON line."""

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
LR, FREQ, K = 0.01, 5, 10
HBM_TBS = 6.3            # achievable HBM rate (tools/bench_metrics.py)
UPDATE = "k_members_update"


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def quiet_optimizer(mode, P, steps):
    from bayesian_inference_for_nn_amd import optimizers
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
    from bayesian_inference_for_nn_amd.nn import sequential_json
    from bayesian_inference_for_nn_amd.nn.model import model_from_json
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    x, y = synth.mnist_like(N_ROWS * 5 // 4, seed=1234)                  # the training split (80 %) has N_ROWS rows
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
    cfg = sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS))
    opt = optimizers.SWAG() if mode == "swag" else optimizers.SGD()
    kw = {"n_members": P} if P > 1 else {}
    opt.compile(HyperParameters(lr=LR, frequency=FREQ, k=K, scale=1.0, batch_size=BATCH), cfg, ds, verbose=False, seed=11,
                starting_model=model_from_json(cfg), **kw)
    opt.train(steps)                                                    # warm-up: buffers, tables
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--modes", nargs="+", default=["swag", "sgd"], choices=["swag", "sgd"])
    ap.add_argument("--no-train", action="store_true", help="skip the quiet train leg")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_members.py needs the GPU"
    x, y = synth.mnist_like(N_ROWS, seed=1234)
    xd, yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    n_tab = max(args.steps, args.warmup, 16)
    idx, sizes = synth.batch_plan(N_ROWS, BATCH, n_tab)
    assert 896 in sizes
    idx_d = torch.as_tensor(idx).cuda()
    lrs = [LR] * n_tab
    stream = torch.cuda.Stream()
    n = args.steps
    out = {"tool": "bench_members", "shape": "784-200-10", "batch": BATCH, "ragged_batch": 896, "steps": n,
           "rounds": args.rounds, "frequency": FREQ, "k": K, "modes": {}}
    base_plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=BATCH)
    D = base_plan.D
    theta0 = torch.as_tensor(synth.glorot_uniform(DIMS)).cuda()
    b_losses = torch.zeros(n_tab, device="cuda")

    def zeros(*shape):
        return torch.zeros(shape, device="cuda")

    legs, plans = {}, {}
    for mode in args.modes:
        swag = mode == "swag"
        b_state = (theta0.clone(), zeros(D), zeros(D), zeros(K, D))

        def baseline(b=b_state, swag=swag):
            with torch.cuda.stream(stream):
                if swag:
                    return events(lambda: base_plan.swag_run(b[0], b[1], b[2], b[3], FREQ, xd, yd, idx_d, sizes[:n], lrs[:n], 0,
                                                             b_losses, use_graph=True)) / n
                return events(lambda: base_plan.sgd_run(b[0], xd, yd, idx_d, sizes[:n], lrs[:n], b_losses, use_graph=True)) / n
        legs[f"{mode}_baseline"] = baseline
        for P in args.members:
            plan = engine.MLPPlan(engine.MLPSpec(DIMS, ACTS, "scce"), max_batch=BATCH, max_particles=P)
            st = {"theta": theta0.repeat(P, 1).contiguous(), "mean": zeros(P, D), "sq": zeros(P, D), "dev": zeros(P, K, D),
                  "loss": zeros(P), "losses": zeros(n_tab, P)}
            plans[mode, P] = (plan, st)

            def one_step(s, hit, col, plan=plan, st=st, swag=swag):
                if swag:
                    plan.swag_members_step(st["theta"], st["mean"], st["sq"], st["dev"], xd, yd, lrs[s], s, hit, col, st["loss"],
                                           batch=sizes[s], row_idx=idx_d[s])
                else:
                    plan.sgd_members_step(st["theta"], st["mean"], xd, yd, lrs[s], s, hit, st["loss"], batch=sizes[s],
                                          row_idx=idx_d[s])
            plans[mode, P] += (one_step,)

            def step_loop(one_step=one_step):
                def body():
                    for s in range(n):
                        hit = s % FREQ == 0
                        one_step(s, hit, min(-(-s // FREQ), K - 1) if hit else None)
                return events(body) / n

            def run(plan=plan, st=st, swag=swag):
                with torch.cuda.stream(stream):
                    if swag:
                        return events(lambda: plan.swag_members_run(st["theta"], st["mean"], st["sq"], st["dev"], FREQ, xd, yd,
                                                                    idx_d, sizes[:n], lrs[:n], 0, st["losses"])) / n
                    return events(lambda: plan.sgd_members_run(st["theta"], st["mean"], FREQ, xd, yd, idx_d, sizes[:n], lrs[:n],
                                                               0, st["losses"])) / n
            legs[f"{mode}_step_loop_p{P}"] = step_loop
            legs[f"{mode}_run_p{P}"] = run
            if not args.no_train:
                opt = quiet_optimizer(mode, P, n)

                def train(opt=opt):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    opt.train(n)
                    return (time.perf_counter() - t0) * 1e6 / n
                legs[f"{mode}_train_p{P}"] = train

    for fn in legs.values():                                             # warm-up of every leg (graph capture, tables)
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            rounds[k].append(fn())
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    for mode in args.modes:
        swag = mode == "swag"
        base = med[f"{mode}_baseline"]
        res = {"baseline": {"entry": "pyz_swag_run" if swag else "pyz_sgd_run", "us_per_step": round(base, 2),
                            "member_steps_per_s": round(1e6 / base, 1)}, "members": {}}
        floats = 8 if swag else 3                                        # a SWAG hit step / an SGD miss step
        for P in args.members:
            plan, st, one_step = plans[mode, P]
            with engine.KernelProbe(256) as kp:                          # 8 steps as the schedule has them
                for s in range(8):
                    hit = s % FREQ == 0
                    one_step(s, hit, min(-(-s // FREQ), K - 1) if hit else None)
            by = kp.by_kernel()
            entry = {"kernels": {name: [c, round(t, 2)] for name, (c, t) in by.items()},
                     "kernel_us_per_step": round(sum(t for _, t in kp.launches) / 8, 2)}
            with engine.KernelProbe(256) as kp:                          # 8 steps of one kind for the update's rate
                for s in range(8):
                    one_step(s, swag, min(s, K - 1) if swag else None)
            upd_us = kp.by_kernel()[UPDATE][1]
            nbytes = floats * 4 * P * D
            entry["update"] = {"step": "swag hit" if swag else "sgd miss", "floats_per_element": floats, "us": round(upd_us, 2),
                               "bytes": nbytes, "tb_per_s": round(nbytes / upd_us * 1e-6, 3),
                               "fraction_of_hbm": round(nbytes / upd_us * 1e-6 / HBM_TBS, 3)}
            for leg in ("step_loop", "run", "train"):
                k = f"{mode}_{leg}_p{P}"
                if k in med:
                    entry[leg] = {"us_per_step": round(med[k], 2), "us_per_member_step": round(med[k] / P, 2),
                                  "member_steps_per_s": round(P * 1e6 / med[k], 1)}
            entry["speedup_run_vs_baseline"] = round(base / (med[f"{mode}_run_p{P}"] / P), 3)
            try:
                plan.check_finite()
            except Exception as e:                                       # a diverged member does not void the timing: say so
                entry["nonfinite"] = str(e)
            res["members"][str(P)] = entry
        out["modes"][mode] = res
    out["rounds_us_per_step"] = {k: [round(t, 2) for t in v] for k, v in rounds.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
