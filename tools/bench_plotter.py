#!/usr/bin/env python3
"""Cost of the Plotter's decision surfaces at plot size (GPU box): the two-moons set of synth.py, a 2 -> 64 -> 64 -> 2
model with a Normal posterior, 100 rows of the test split, granularity 1e-3 (a 1000 x 1000 grid: 10^6 rows).
    uncertainty_area_ms        Plotter.uncertainty_area_data: 100 weight draws, top / cls / ent per grid row come back
                               (wall clock around a call that ends in the download, median of --rounds)
    decision_boundaries_ms     Plotter.decision_boundaries_data: 10 draws, one column per draw comes back (40 MB)
    kernels                    {kernel: [launches, mean us]} of one uncertainty_area_data call (KernelProbe)
    k_predict_surface          its summed time, the bytes it moves (reads draws * rows * C floats, writes rows * (C + 3)),
                               bytes / s and the fraction of the 6.3 TB/s achievable HBM rate
    baseline                   the same arrays from a grid built on the host (NumPy float32), uploaded and read out with
                               BayesianModel.predict -- the (draws, rows, C) sample tensor formed and copied back -- in
                               the same process, alternating with the timed calls
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
from bayesian_inference_for_nn_amd.distributions import tfd  # noqa: E402
from bayesian_inference_for_nn_amd.distributions.tf import TensorflowProbabilityDistribution  # noqa: E402
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy  # noqa: E402
from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json  # noqa: E402
from bayesian_inference_for_nn_amd.visualisations import Plotter  # noqa: E402
from bayesian_inference_for_nn_amd.visualisations.Plotter import grid_axes, grid_mesh  # noqa: E402

DIMS, ACTS = (2, 64, 64, 2), ("relu", "relu", "softmax")
ROWS, DRAWS, BOUNDARIES, GRANULARITY, THRESHOLD = 100, 100, 10, 1e-3, 0.9
HBM_TBS = 6.3            # achievable HBM rate


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _host_grid(x):
    a0, da, n1, b0, db, n2 = grid_axes(x, GRANULARITY, 0.2)
    dim1, dim2 = grid_mesh(a0, da, n1, b0, db, n2)
    return np.stack([dim1.reshape(-1), dim2.reshape(-1)], axis=1), dim1.shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_plotter.py needs the GPU"
    x, y = synth.moons(2000, seed=42)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", train_proportion=0.0, test_proportion=1.0,
                 valid_proportion=0.0, seed=0)
    bm = BayesianModel(sequential_json(DIMS[0], list(DIMS[1:]), list(ACTS)))
    loc = synth.glorot_uniform(DIMS).astype(np.float32)
    bm.apply_distribution(TensorflowProbabilityDistribution(tfd.Normal(loc, np.full_like(loc, 0.05))), 0, 2)
    tfd.seed(3)
    pl = Plotter(bm, ds)
    xt = np.asarray(ds.test_data.as_numpy()[0][:ROWS], dtype=np.float32)

    def area():
        return pl.uncertainty_area_data(granularity=GRANULARITY, n_samples=ROWS, uncertainty_threshold=THRESHOLD)

    def boundaries():
        return pl.decision_boundaries_data(granularity=GRANULARITY, n_samples=ROWS)

    def area_baseline():
        grid, shape = _host_grid(xt)
        _, mean = bm.predict(grid, DRAWS)
        top = np.asarray(mean).max(axis=1).reshape(shape)
        return top, (top < np.float32(THRESHOLD)).astype(np.float32)

    def boundaries_baseline():
        grid, shape = _host_grid(xt)
        samples, _ = bm.predict(grid, BOUNDARIES)
        return np.stack([np.asarray(s)[:, 0].reshape(shape) for s in samples])

    legs = {"uncertainty_area": area, "uncertainty_area_baseline": area_baseline, "decision_boundaries": boundaries,
            "decision_boundaries_baseline": boundaries_baseline}
    ms = {k: [] for k in legs}
    out = {}
    for i in range(args.rounds + 1):       # the first round builds the plans and is dropped; the legs alternate
        for k, fn in legs.items():
            dt, out[k] = _wall(fn)
            if i:
                ms[k].append(dt)
    n_grid = out["uncertainty_area"]["top"].size
    assert out["uncertainty_area"]["top"].shape == out["uncertainty_area_baseline"][0].shape
    assert out["decision_boundaries"]["boundaries"].shape == out["decision_boundaries_baseline"].shape

    with engine.KernelProbe(4096) as kp:
        area()
    split = {name: [c, round(t, 2)] for name, (c, t) in kp.by_kernel().items()}
    ps_us = sum(t for name, t in kp.launches if name == "k_predict_surface")
    C = DIMS[-1]
    nbytes = 4.0 * (DRAWS * n_grid * C + n_grid * (C + 3))
    tbs = nbytes / (ps_us * 1e-6) / 1e12

    med = {k: round(float(np.median(v)), 1) for k, v in ms.items()}
    res = {"tool": "bench_plotter", "shape": "2-64-64-2", "grid_rows": int(n_grid), "rows": ROWS, "draws": DRAWS,
           "boundaries": BOUNDARIES, "granularity": GRANULARITY, "rounds": args.rounds,
           "uncertainty_area_ms": med["uncertainty_area"], "decision_boundaries_ms": med["decision_boundaries"],
           "ms_rounds": {k: [round(v, 1) for v in vs] for k, vs in ms.items()},
           "kernels": split, "kernel_us_total": round(sum(t for _, t in kp.launches), 1), "launches": len(kp.launches),
           "k_predict_surface": {"us": round(ps_us, 1), "mbytes": round(nbytes / 1e6, 1), "tb_per_s": round(tbs, 3),
                                 "hbm_tb_per_s": HBM_TBS, "fraction_of_hbm": round(tbs / HBM_TBS, 4)},
           "baseline": {"uncertainty_area_ms": med["uncertainty_area_baseline"],
                        "decision_boundaries_ms": med["decision_boundaries_baseline"],
                        "kind": "host-built float32 grid, uploaded, BayesianModel.predict with the sample tensor copied back"}}
    res["speedup_uncertainty_area"] = round(med["uncertainty_area_baseline"] / med["uncertainty_area"], 1)
    res["speedup_decision_boundaries"] = round(med["decision_boundaries_baseline"] / med["decision_boundaries"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
