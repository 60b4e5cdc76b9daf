#!/usr/bin/env python3
"""Cost of one SWAG step of a conv model (GPU box): the model of the reference's image script (tests/tf_dataset_test.py:42-57),
32 x 32 x 3 -> Conv2D(32, 3, same, relu) -> Flatten -> Dense(50, relu) -> Dense(10, softmax), batch 128 of 2048 synthetic
images, k = 20 deviation rows, frequency 1.  A first measurement: no bar.
    swag_step_us           pyz_convnet_swag_step (device events around --steps steps after --warmup; median of --rounds)
    kernels                {kernel: [launches, mean us]} of one step (KernelProbe)
    conv                   per conv kernel: the FLOPs its GEMM needs (2 M (K + 1) N, from the shapes), its time, FLOP/s and
                           the share of the fp32-MFMA peak (155 TF measured, MI355X_MICROARCH.md)
    torch_eager_step_us    the same step written in torch-ROCm eager float32 (F.conv2d, TF32 off) on the same GPU, timed
                           the same way; ratio = torch_eager_step_us / swag_step_us
Prints one JSON line."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bayesian_inference_for_nn_amd import engine  # noqa: E402
from bayesian_inference_for_nn_amd.nn.model import conv_sequential_json, model_from_json  # noqa: E402

SIDE, CIN, FILTERS, BATCH, ROWS, K_DEV = 32, 3, 32, 128, 2048, 20
MFMA_F32_TFLOPS = 155.0


def _events(fn, steps, rounds):
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(steps):
            fn(s)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / steps)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv.py needs the GPU"
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    net = model_from_json(conv_sequential_json((SIDE, SIDE, CIN), [("conv", FILTERS, 3, "same", "relu")], (50, 10),
                                               ("relu", "softmax")))
    net.reset_glorot(np.random.default_rng(0))
    spec = engine.ConvSpec(net.spec.input_shape, net.spec.ops, engine.MLPSpec(net.dims, net.acts, "scce"))
    rng = np.random.default_rng(1)
    x = rng.normal(size=(ROWS, SIDE * SIDE * CIN)).astype(np.float32)
    y = rng.integers(0, 10, size=ROWS).astype(np.int32)
    idx = torch.as_tensor(np.stack([rng.permutation(ROWS)[:BATCH] for _ in range(64)]).astype(np.int32)).cuda()
    xd, yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    plan = engine.ConvPlan(spec, max_batch=BATCH)
    D, lr = plan.D, 1e-3
    theta = torch.as_tensor(net.weights_flat.copy()).cuda()
    mean, sq = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    dev = torch.zeros((K_DEV, D), device="cuda")
    loss = torch.zeros(1, device="cuda")
    count = [0]

    def step(s):
        n = count[0]
        plan.swag_step(theta, mean, sq, dev[min(n, K_DEV - 1)], xd, yd, lr, n, True, loss, batch=BATCH, row_idx=idx[s % 64])
        count[0] += 1

    for s in range(args.warmup):
        step(s)
    torch.cuda.synchronize()
    ours = _events(step, args.steps, args.rounds)
    with engine.KernelProbe(64) as kp:
        step(0)
    split = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}
    M, Kc, N = BATCH * SIDE * SIDE, 9 * CIN, FILTERS
    flops = 2.0 * M * (Kc + 1) * N
    conv = {}
    for name in ("k_conv_fwd", "k_conv_wgrad"):
        us = sum(t for nm, t in kp.launches if nm == name)
        conv[name] = {"us": round(us, 2), "gflop": round(flops / 1e9, 3), "tflops": round(flops / (us * 1e-6) / 1e12, 2),
                      "share_of_mfma_f32_peak": round(flops / (us * 1e-6) / 1e12 / MFMA_F32_TFLOPS, 4)}

    # the same step in torch eager float32
    kh = 3
    n_k = kh * kh * CIN * FILTERS
    th = torch.as_tensor(net.weights_flat.copy()).cuda()
    sl = spec.layer_slices()
    xi = xd.reshape(ROWS, SIDE, SIDE, CIN).permute(0, 3, 1, 2).contiguous()
    yl = yd.long()
    t_mean, t_sq, t_dev = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros((K_DEV, D), device="cuda")
    t_count = [0]

    def torch_step(s):
        w = th.detach().requires_grad_(True)
        rows = idx[s % 64].long()
        k = w[:n_k].reshape(kh, kh, CIN, FILTERS).permute(3, 2, 0, 1)
        h = torch.relu(F.conv2d(xi[rows], k, w[n_k:sl[0].stop], padding="same"))
        a = h.permute(0, 2, 3, 1).reshape(BATCH, -1)
        for li, act in ((1, "relu"), (2, None)):
            i, o = spec.variable_shapes()[li][0]
            a = a @ w[sl[li].start:sl[li].start + i * o].reshape(i, o) + w[sl[li].start + i * o:sl[li].stop]
            if act:
                a = torch.relu(a)
        g, = torch.autograd.grad(F.cross_entropy(a, yl[rows]), w)
        n = float(t_count[0])
        with torch.no_grad():
            th.sub_(lr * g)
            t_mean.mul_(n).add_(th).div_(n + 1.0)
            t_sq.mul_(n).addcmul_(th, th).div_(n + 1.0)
            t_dev[min(t_count[0], K_DEV - 1)] = th - t_mean
        t_count[0] += 1

    for s in range(args.warmup):
        torch_step(s)
    torch.cuda.synchronize()
    theirs = _events(torch_step, args.steps, args.rounds)
    res = {"tool": "bench_conv", "model": f"{SIDE}x{SIDE}x{CIN}-conv{FILTERS}k3same-50-10", "batch": BATCH, "k": K_DEV,
           "params": D, "steps": args.steps, "rounds": args.rounds,
           "swag_step_us": round(float(np.median(ours)), 1), "swag_step_us_rounds": [round(v, 1) for v in ours],
           "kernels": split, "kernel_us_total": round(sum(t for _, t in kp.launches), 1), "conv": conv,
           "torch_eager_step_us": round(float(np.median(theirs)), 1), "torch_eager_step_us_rounds": [round(v, 1) for v in theirs],
           "workspace_mb": round(plan.workspace_bytes / 1e6, 1)}
    res["ratio_torch_over_ours"] = round(res["torch_eager_step_us"] / res["swag_step_us"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
