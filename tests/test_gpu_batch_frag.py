"""Device-resident SGD / SWAG / SGLD runs keep the batch assembled ahead of each step as two fragment-major images
(csrc/pyz_fused.h PrepArgs: one in the order k_dense_fwd_frag's A fragments read it, one in the order layer 0 of
k_wgrad_all_frag reads it) instead of one row-major copy.  The images feed the same operand values to the same MFMAs in
the same order, so a run with images must equal the same run with PYZ_BATCH_FRAG=0 BIT FOR BIT: theta, mean, sq_mean (and
SWAG's deviation rows) and every loss.  The switch is read when a plan is created, so each comparison builds two plans in
this process, one under each setting, and asks each which form its run used (MLPPlan.run_batch_form).

Shapes: the smallest at which the indexing of the images can go wrong --
  input width K   8 (one chunk, a quarter column block), 40 (one and a quarter column blocks), 72 (more than two)
  batch           8 (one row group), 34 (row block and row group partial, odd step count), 64, 70 (wave ranges of the
                  weight-gradient reduction that are no multiples of four steps); 1, 2, 4 and 4 waves per weight-gradient tile
  hidden width N  8, 40 (one and two column tiles)
  run length      1 (the first batch alone, k_run_start_frag), 2 (both slots), 3, 33 (a graph chunk and its remainder)
The full product runs, in every mode (a comparison takes milliseconds).  Two further shapes reach 16 waves per tile in both
kernels (K = 264, batch 256 and 262: aligned and unaligned wave ranges); the table's own shapes cover 1, 2 and 4.  No
tolerance anywhere: array_equal."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import mlp as o_mlp


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


@pytest.fixture(scope="module")
def eng(gpu_device):
    from bayesian_inference_for_nn_amd import engine
    return engine


def plan_with_switch(eng, spec, max_batch, on):
    """A plan created under PYZ_BATCH_FRAG=on (read once, when the plan is created); the environment is put back."""
    old = os.environ.get("PYZ_BATCH_FRAG")
    os.environ["PYZ_BATCH_FRAG"] = "1" if on else "0"
    try:
        return eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=max_batch)
    finally:
        if old is None:
            del os.environ["PYZ_BATCH_FRAG"]
        else:
            os.environ["PYZ_BATCH_FRAG"] = old


def tables(rng, n_rows, max_batch, sizes):
    """Row table (steps, max_batch): step s uses sizes[s] distinct rows; the entries behind them name other (valid) rows,
    which no step may use."""
    idx = rng.integers(0, n_rows, size=(len(sizes), max_batch)).astype(np.int32)
    for s, b in enumerate(sizes):
        idx[s, :b] = rng.permutation(n_rows)[:b]
    return idx


def run(eng, spec, mode, on, max_batch, sizes, x, y, idx, theta0, seed=7):
    """One resident run from theta0 on a fresh plan; returns (the arrays of the result, the batch form the run used)."""
    n, D = len(sizes), spec.n_params
    plan = plan_with_switch(eng, spec, max_batch, on)
    xd, yd, idxd = dev(x), dev(y, torch.int32), dev(idx, torch.int32)
    th, mean, sq = dev(theta0), torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    losses = torch.zeros(n, device="cuda")
    lrs = [0.02 / (1 + s) for s in range(n)]
    extra = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        if mode == "sgld":
            plan.sgld_run(th, mean, sq, xd, yd, idxd, sizes, lrs, 0, seed, losses, use_graph=True)
        elif mode == "sgd":
            plan.sgd_run(th, xd, yd, idxd, sizes, lrs, losses, use_graph=True)
        elif mode == "swag":
            devm = torch.zeros(3, D, device="cuda")
            plan.swag_run(th, mean, sq, devm, 2, xd, yd, idxd, sizes, lrs, 0, losses, use_graph=True)
            extra = [devm]
        else:
            m, v = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
            plan.adam_run(th, m, v, xd, yd, idxd, sizes, lrs, [1 + s for s in range(n)], 0.9, 0.999, losses, use_graph=True)
            extra = [m, v]
    stream.synchronize()
    plan.check_finite()
    form = plan.run_batch_form()
    out = [t.cpu().numpy().copy() for t in [th, mean, sq, losses] + extra]
    plan.close()
    return out, form


def problem(k_in, n_hidden, n_rows, seed):
    spec = o_mlp.MLPSpec((k_in, n_hidden, 4), ("relu", "softmax"), "scce")
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n_rows, k_in)).astype(np.float32)
    y = rng.integers(0, 4, size=n_rows).astype(np.int32)
    theta0 = (rng.normal(size=spec.n_params) * 0.3).astype(np.float32)
    return spec, rng, x, y, theta0


def compare(eng, spec, mode, max_batch, sizes, x, y, idx, theta0, want_on):
    a, form_on = run(eng, spec, mode, True, max_batch, sizes, x, y, idx, theta0)
    b, form_off = run(eng, spec, mode, False, max_batch, sizes, x, y, idx, theta0)
    assert form_off == "rows", form_off
    assert form_on == want_on, form_on
    names = ("theta", "mean", "sq_mean", "losses", "extra0", "extra1")
    for u, v, name in zip(a, b, names):
        assert np.array_equal(u, v), f"{mode} {name}: images and rows differ (max {np.abs(u - v).max():.3e})"
    assert np.isfinite(a[3]).all() and not np.array_equal(a[0], theta0)     # the run ran


K_INS, BATCHES, HIDDEN, LENGTHS, MODES = (8, 40, 72), (8, 34, 64, 70), (8, 40), (1, 2, 3, 33), ("sgld", "sgd", "swag")


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("k_in", K_INS)
def test_images_equal_rows_bit_for_bit(eng, k_in, batch):
    """Every hidden width, run length and mode at this (K, batch): 24 comparisons of a few milliseconds each."""
    for n_hidden in HIDDEN:
        spec, rng, x, y, theta0 = problem(k_in, n_hidden, 3 * batch + 5, 1000 * k_in + 10 * batch + n_hidden)
        for n_steps in LENGTHS:
            sizes = [batch] * n_steps
            idx = tables(rng, x.shape[0], batch, sizes)
            for mode in MODES:
                compare(eng, spec, mode, batch, sizes, x, y, idx, theta0, "images")


@pytest.mark.parametrize("batch", [256, 262])
def test_sixteen_waves_per_tile(eng, batch):
    """K = 264, batch >= 256: both kernels split their reduction over 16 waves (262: 131 steps, ranges of 8 or 9)."""
    spec, rng, x, y, theta0 = problem(264, 40, batch + 40, batch)
    sizes = [batch] * 3
    idx = tables(rng, x.shape[0], batch, sizes)
    compare(eng, spec, "sgld", batch, sizes, x, y, idx, theta0, "images")


@pytest.mark.parametrize("mode", MODES)
def test_ragged_run(eng, mode):
    """The last batch of every epoch is smaller than the launch's (64, 64, 22 and 64, 63, 3): rows and row groups of the
    images past the step's batch hold the previous batches' values, or nothing."""
    spec, rng, x, y, theta0 = problem(40, 40, 150, 5)
    sizes = [64, 64, 22, 64, 63, 3, 64]
    idx = tables(rng, x.shape[0], 64, sizes)
    compare(eng, spec, mode, 64, sizes, x, y, idx, theta0, "images")


def test_fallback_shapes_take_the_row_major_copy(eng):
    """K = 23 (no multiple of 8) and an ADAM run (k_wgrad_adam reads rows) keep the row-major copy with the switch on."""
    spec, rng, x, y, theta0 = problem(23, 16, 101, 11)
    sizes = [34] * 3
    compare(eng, spec, "sgld", 34, sizes, x, y, tables(rng, x.shape[0], 34, sizes), theta0, "rows")
    spec, rng, x, y, theta0 = problem(24, 16, 101, 12)
    compare(eng, spec, "adam", 34, sizes, x, y, tables(rng, x.shape[0], 34, sizes), theta0, "rows")
