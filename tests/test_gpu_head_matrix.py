"""Every loss-head kernel variant against the float64 oracle (tests/head_cases.py lists the cases).

Each case first checks that `loss_grad` launched the head kernel its shape selects, so a change in dispatch fails
the case instead of quietly testing another kernel; then the loss and gradient of the first, middle and last
particle (each layer's W and b block on its own scale), the forward pass, and the loss-only call."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from head_cases import CASES, case_data, check_particles, close_blocks  # noqa: E402
from oracle import mlp as o_mlp  # noqa: E402


@pytest.fixture(scope="module")
def eng(gpu_device):
    from bayesian_inference_for_nn_amd import engine
    return engine


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def dev_x(x, offset):
    """x on the device; with `offset` as a contiguous view 4 bytes into its storage (no 16-byte aligned loads)."""
    if not offset:
        return dev(x)
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    buf[1:].copy_(dev(x).reshape(-1))
    xd = buf[1:].view(x.shape)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    return xd


def check_forward(out, ref, scce, what):
    out = out.cpu().numpy().astype(np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    scale = np.abs(ref).max()
    err = np.abs(out - ref).max()
    assert err <= 1e-4 * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"
    if scce:
        # the predicted class exactly; a row whose two best classes lie within the value tolerance may pick either
        pick, best = out.argmax(1), ref.argmax(1)
        rows = np.arange(len(ref))
        tied = ref[rows, best] - ref[rows, pick] <= 1e-4 * scale
        assert np.all((pick == best) | tied), f"{what}: argmax differs in rows {np.flatnonzero((pick != best) & ~tied)}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_head_case(eng, case):
    spec, P, B = case.spec, case.P, case.batch
    x, y, idx, thetas = case_data(case)
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=B + 5, max_particles=P)
    xd = dev_x(x, case.extra.get("x_offset"))
    yd = dev(y, torch.int32 if spec.loss == "scce" else torch.float32)
    rid = dev(idx, torch.int32) if idx is not None else None
    th = dev(thetas)
    with eng.KernelProbe(32) as kp:
        loss, grad = plan.loss_grad(th, xd, yd, batch=B, row_idx=rid)
    names = [n.replace(" ", "") for n, _ in kp.launches]
    assert case.kernel.replace(" ", "") in names, (case.kernel, kp.launches)
    out = plan.forward(th, xd, batch=B, row_idx=rid)
    loss_only, none = plan.loss_grad(th, xd, yd, batch=B, row_idx=rid, want_grad=False)
    assert none is None
    loss, loss_only = loss.cpu().numpy(), loss_only.cpu().numpy()
    rows, ys = (x, y) if idx is None else (x[idx], y[idx])
    for p in check_particles(P):
        rl, rg, rout = o_mlp.loss_and_grad(thetas[p], rows, ys, spec)
        for what, v in (("loss", loss[p]), ("loss only", loss_only[p])):
            assert abs(float(v) - rl) <= 1e-4 * abs(rl), f"{case.name} {what}[{p}]: {float(v)!r} vs {rl!r}"
        close_blocks(grad[p], rg, spec, what=f"{case.name} grad[{p}]")
        check_forward(out[p], rout, spec.loss == "scce", f"{case.name} forward[{p}]")
    plan.close()
