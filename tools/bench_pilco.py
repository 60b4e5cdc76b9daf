#!/usr/bin/env python3
"""Cost of one Deep-PILCO policy update (GPU box): PilcoPlan.policy_step, Adam on, on seeded inputs of a case of
tests/pilco_checks.py (default `example`: K = 32, H = 32, policy 6 -> 80 -> 3, dynamics 9 -> 512 -> 256 -> 6) or of
tests/pilco_rbf_checks.py (`rbf_example`: the same shape with the policy's hidden layer RBF(80, 0.5)).
    graph_ms / plain_ms   ms per update through the captured graph and through plain launches: --updates updates after
                          --warmup ones, host clock around calls that end in a stream synchronise, --rounds rounds per path,
                          the two paths alternating in one process
    kernels               {kernel: [launches, mean us]} of one plain update (KernelProbe) and their sum
    workspace_mib         the plan's tape and scratch
Prints one JSON line."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import pilco_checks as pc  # noqa: E402
import pilco_rbf_checks as rc  # noqa: E402
from bayesian_inference_for_nn_amd.engine import KernelProbe, MLPSpec, PilcoPlan  # noqa: E402
from bayesian_inference_for_nn_amd.nn.model import PolicyNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="example", choices=[c.name for c in pc.CASES + rc.CASES])
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pilco needs the GPU: a CPU run says nothing about it")
    if a.case in rc.CASE:
        case = rc.CASE[a.case]
        inputs, policy = rc.make_inputs(case), PolicyNet(case.S, case.pol_hidden, case.A, case.pol_out)
    else:
        case = pc.CASE[a.case]
        inputs, policy = pc.make_inputs(case), MLPSpec(case.pol_dims, case.pol_acts, "mse")
    d = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in inputs.items()}
    plan = PilcoPlan(policy, MLPSpec(case.dyn_dims, case.dyn_acts, "mse"), case.K, case.H)
    phi, m, v = d["phi"].clone(), torch.zeros_like(d["phi"]), torch.zeros_like(d["phi"])

    def update(t, use_graph):
        plan.policy_step(phi, m, v, t, d["W"], d["s0"], d["eps"], case.H, pc.GAMMA, case.reward, lr=1e-3, use_graph=use_graph)

    stream = torch.cuda.Stream()                    # (the legacy default stream cannot be captured)
    stream.wait_stream(torch.cuda.current_stream())
    ms = {True: [], False: []}
    with torch.cuda.stream(stream):
        for _ in range(a.rounds):
            for use_graph in (True, False):
                for t in range(1, a.warmup + 1):
                    update(t, use_graph)
                stream.synchronize()
                t0 = time.perf_counter()
                for t in range(a.warmup + 1, a.warmup + 1 + a.updates):
                    update(t, use_graph)
                stream.synchronize()
                ms[use_graph].append(round((time.perf_counter() - t0) / a.updates * 1e3, 4))
        with KernelProbe(4 * case.H + 16) as kp:
            update(a.warmup + 1, False)
    out = {"tool": "bench_pilco", "case": case.name, "K": case.K, "H": case.H, "policy": list(case.pol_dims),
           "policy_kinds": list(getattr(case, "pol_kinds", ("dense",) * len(case.pol_acts))),
           "dynamics": list(case.dyn_dims), "updates": a.updates, "warmup": a.warmup,
           "graph_ms": float(np.median(ms[True])), "plain_ms": float(np.median(ms[False])),
           "ms_rounds": {"graph": ms[True], "plain": ms[False]},
           "kernels": {k: [c, round(us, 2)] for k, (c, us) in sorted(kp.by_kernel().items())},
           "kernel_us_total": round(sum(us for _, us in kp.launches), 1), "launches": len(kp.launches),
           "workspace_mib": round(plan.workspace_bytes / 2 ** 20, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
