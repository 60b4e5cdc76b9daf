"""The conv kernels' paths that no row of the case table reaches, at shapes made for them (conv_checks.PATH_SHAPES; the
arithmetic that puts each shape on its path is tests/test_conv_dispatch_table.py's, and is asserted again here):

  a  weight-gradient ranges of several chunks with every row live: the chunk loop of k_conv_wgrad, its barrier, the
     rebuilt corner / yx table, a second chunk of 8 rows and an odd one of 115;
  b  16 777 215 rows, one short of PYZ_CONV_MAX_ROWS: pyz_fdiv's (b, oy, ox) near 2^24, 256 ranges of 128 chunks;
  c  one plan over batches 33, 1, 7, 33: nothing of an earlier, larger call is read.

Tolerance: 1e-4 of the reference block's largest magnitude, as everywhere."""

import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_checks as cc  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def draw_theta(spec, rng):
    """Kernels of unit-variance pre-activations, biases of 0.3 (the rule of conv_checks._draw)."""
    theta = np.empty(spec.n_params, dtype=np.float32)
    for sl, (ks, bs) in zip(spec.layer_slices(), spec.variable_shapes()):
        n, fan_in = int(np.prod(ks)), int(np.prod(ks[:-1]))
        theta[sl.start:sl.start + n] = rng.normal(size=n) / np.sqrt(fan_in)
        theta[sl.start + n:sl.stop] = 0.3 * rng.normal(size=bs[0])
    return theta


# ---------------------------------------------------------------- a. ranges of several chunks
@pytest.mark.parametrize("name,batch", [("a1", 5), ("a1", 130), ("a2", 3)])
def test_ranges_of_several_chunks(gpu_device, name, batch):
    from bayesian_inference_for_nn_amd.engine import ConvPlan
    case, max_batch = cc.path_case(name)
    spec = case.spec()
    # the path, from the restatement of the launch rules: a later change of the range rule fails here, loudly
    (L,) = cc.conv_launches(case.shape, case.ops, batch, max_batch)
    (tight,) = cc.conv_launches(case.shape, case.ops, batch, batch + cc.PLAN_SLACK)
    if name == "a1":
        assert L.rows_per_g == 520 and all(r == (512, 8) for r in L.chunks[:-1]) and L.wgrad_S == 4
        assert L.chunks[-1] == ((512, 8) if batch == 130 else (440,)) and L.G == (256 if batch == 130 else 10)
    else:
        assert (L.M, L.rows_per_g, L.G) == (2883, 752, 4) and L.chunks[-1] == (512, 115) and L.chunks[0] == (512, 240)
    if batch < 130:
        assert tight.rows_per_g == 256 and all(len(r) == 1 for r in tight.chunks)      # the tight plan: single-chunk ranges
    rng = np.random.default_rng([3, batch, ord(name[1])])
    rows = batch + cc.EXTRA_ROWS
    x = rng.normal(size=(rows, int(np.prod(case.shape)))).astype(np.float32)
    y = rng.integers(0, case.units[-1], size=rows).astype(np.int32)
    idx = rng.permutation(rows)[:batch].astype(np.int32)
    theta = draw_theta(spec, rng)
    ref = cc.loss_grad(spec, theta.astype(np.float64), x[idx].astype(np.float64), y[idx])
    x[np.setdiff1d(np.arange(rows), idx)] = np.nan            # every image outside the batch
    th, xd, yd, idxd = dev(theta), dev(x), dev(y), dev(idx)
    got = {}
    for which, mb in (("wide", max_batch), ("tight", batch + cc.PLAN_SLACK)):
        plan = ConvPlan(spec, max_batch=mb)
        feat = plan.stem_forward(th, xd, batch=batch, row_idx=idxd)
        loss, grad = plan.loss_grad(th, xd, yd, batch=batch, row_idx=idxd)
        torch.cuda.synchronize()
        e = cc.errors(float(loss[0]), grad[0].cpu().numpy(), feat[0].cpu().numpy(), ref, spec)
        cc.assert_close(e, f"{name} batch {batch}, {which} plan (max_batch {mb}): rows through row_idx")
        loss2, grad2 = plan.loss_grad(th, xd, yd, batch=batch, row_idx=idxd)
        assert np.array_equal(bits(grad), bits(grad2)) and np.array_equal(bits(loss), bits(loss2)), f"{which}: a repeated call changed bits"
        got[which] = grad[0].cpu().numpy()
        plan.check_finite()
        plan.close()
    # the two splits of the same sum agree within the bound (not in bits: the order of the additions differs)
    cc.assert_close(cc.block_errors(got["wide"], got["tight"], spec), f"{name} batch {batch}: wide plan against tight plan")


# ---------------------------------------------------------------- b. rows up to 2^24
def test_rows_one_short_of_the_cap(gpu_device):
    """4097 images of 63 x 65: 16 777 215 rows.  Images are independent, so the features of five of them and the stem
    gradient of a feature gradient that is zero on all others have a float64 reference of five images."""
    from bayesian_inference_for_nn_amd.engine import ConvPlan
    t0 = time.time()
    case, max_batch = cc.path_case("b")
    spec = case.spec()
    (L,) = cc.conv_launches(case.shape, case.ops, max_batch, max_batch)
    assert L.M == cc.CONV_MAX_ROWS - 1 and L.G == 256 and all(len(r) == 128 for r in L.chunks) and L.chunks[-1][-1] == 511
    live = np.array([0, 1, 2048, 4095, 4096])
    n_in, F = int(np.prod(case.shape)), spec.features
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    x = torch.randn((max_batch, n_in), generator=gen, device="cuda", dtype=torch.float32)
    rng = np.random.default_rng(17)
    theta = draw_theta(spec, rng)
    x5 = x[torch.as_tensor(live).cuda()].cpu().numpy().astype(np.float64)
    d5 = rng.normal(size=(len(live), F))
    f = cc.forward(spec, theta.astype(np.float64), x5)
    ref_grad = cc.stem_grad(f, d5.astype(np.float32).astype(np.float64))
    plan = ConvPlan(spec, max_batch=max_batch)
    th = dev(theta)
    feat = plan.stem_forward(th, x)
    dfeat = torch.zeros((1, max_batch, F), dtype=torch.float32, device="cuda")
    dfeat[0, torch.as_tensor(live).cuda()] = dev(d5.astype(np.float32))
    g = plan.stem_backward(th, x, dfeat)
    torch.cuda.synchronize()
    e = {f"features of image {b}": cc.rel(feat[0, b].cpu().numpy(), f["features"][i]) for i, b in enumerate(live)}
    n = int(np.prod(spec.variable_shapes()[0][0]))
    got = g[0].cpu().numpy().astype(np.float64)
    e["W0"] = cc.rel(got[:n], ref_grad[:n])
    e["b0"] = cc.rel(got[n:], ref_grad[n:])
    assert np.abs(ref_grad[:n]).max() > 0 and np.abs(ref_grad[n:]).max() > 0
    cc.assert_close(e, f"b: {L.M} rows, stem entry points")
    g2 = plan.stem_backward(th, x, dfeat)
    assert np.array_equal(bits(g), bits(g2)), "a repeated stem_backward changed bits"
    plan.close()
    print(f"b: {time.time() - t0:.2f} s")


# ---------------------------------------------------------------- c. one plan, changing batches
def test_one_plan_over_changing_batches(gpu_device):
    """Case C's model (conv, pool, conv) on one plan of max_batch 36, batches 33, 1, 7, 33 of different rows, NaN in
    every image outside the batch: each result equals, bit for bit, that of a fresh plan that has seen only that batch --
    so nothing of the rows an earlier, larger call left in out / delta / win / the partial-tile slab is read."""
    from bayesian_inference_for_nn_amd.engine import ConvPlan
    case = cc.CASES["C"]
    spec = case.spec()
    rng = np.random.default_rng(23)
    rows = 80
    x0 = rng.normal(size=(rows, int(np.prod(case.shape)))).astype(np.float32)
    y = rng.integers(0, case.units[-1], size=rows).astype(np.int32)
    theta = dev(draw_theta(spec, rng))
    yd = dev(y)
    order = rng.permutation(rows)
    shared = ConvPlan(spec, max_batch=36)
    at = 0
    for k, batch in enumerate((33, 1, 7, 33)):
        idx = order[at:at + batch].astype(np.int32)          # different rows each time
        at += batch
        assert len(idx) == batch and at <= rows
        x = x0.copy()
        x[np.setdiff1d(np.arange(rows), idx)] = np.nan
        xd, idxd = dev(x), dev(idx)
        fresh = ConvPlan(spec, max_batch=36)
        res = []
        for plan in (shared, fresh):
            feat = plan.stem_forward(theta, xd, batch=batch, row_idx=idxd)
            loss, grad = plan.loss_grad(theta, xd, yd, batch=batch, row_idx=idxd)
            torch.cuda.synchronize()
            res.append((bits(feat), bits(loss), bits(grad)))
            assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and torch.isfinite(feat).all(), (k, batch)
        for a, b, what in zip(res[0], res[1], ("features", "loss", "grad")):
            assert np.array_equal(a, b), f"call {k} (batch {batch}): {what} of the used plan differs from a fresh plan's"
        fresh.close()
    shared.close()
