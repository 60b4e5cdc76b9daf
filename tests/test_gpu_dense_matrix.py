"""Every Dense GEMM kernel variant against the float64 oracle (tests/dense_cases.py lists the cases and the cells).

Each case first checks that the call launched the kernels its shape selects (forward kernels in layer order, the number
of data-gradient launches, the weight-gradient expressions), so a change in dispatch fails the case instead of quietly
testing another kernel; then loss, gradient (each layer's W and b block on its own scale), forward and the loss-only
call of the first, middle and last particle against oracle.mlp; then that a second call returns the same bits (the
kernels combine partial tiles in a fixed order and use no atomics); and, without a gather, that a batch one row shorter
on the same plan and the same x leaves the rows past it alone."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from dense_cases import (CASES, ENV_FORBIDDEN, batch_rows, case_data, check_particles,  # noqa: E402
                         expected_launches)
from head_cases import close_blocks  # noqa: E402
from oracle import mlp as o_mlp  # noqa: E402
from oracle import sgd as o_sgd  # noqa: E402

PER_CALL_ENV = ("PYZ_FWD_LDS", "PYZ_FWD_LDS_MINWG")
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in ENV_FORBIDDEN if os.environ.get(k)]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the library reads them once per process and every "
                    "expected launch of this module assumes their defaults -- unset them")
    from bayesian_inference_for_nn_amd import engine
    return engine


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def dev_x(x, offset):
    """x on the device; with `offset` as a contiguous view 4 bytes into its storage (no 16-byte aligned loads)."""
    if not offset:
        xd = dev(x)
        assert xd.data_ptr() % 16 == 0
        return xd
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    buf[1:].copy_(dev(x).reshape(-1))
    xd = buf[1:].view(x.shape)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    return xd


def check_forward(out, ref, what):
    out = out.cpu().numpy().astype(np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.all(np.isfinite(out)), f"{what}: non-finite outputs"
    scale = np.abs(ref).max()
    diff = np.abs(out - ref)
    err = diff.max()
    at = tuple(map(int, np.unravel_index(int(diff.argmax()), ref.shape)))
    print(f"{what}: max err {err:.3e} at {at}, scale {scale:.3e}")
    assert err <= 1e-4 * scale, f"{what}: max err {err:.3e} at {at} vs scale {scale:.3e}"


def check_loss(v, ref, what):
    print(f"{what}: {float(v)!r} vs {ref!r}")
    assert abs(float(v) - ref) <= 1e-4 * abs(ref), f"{what}: {float(v)!r} vs {ref!r}"


def launched(kp):
    """The Dense launches of a probed call, per family, spaces removed."""
    names = [n.replace(" ", "") for n, _ in kp.launches]
    return ([n for n in names if n.startswith("k_dense_fwd")], sum(n == "k_dense_bwd_data" for n in names),
            [n for n in names if "k_wgrad_all" in n or n.startswith("k_dense_bwd_weight")])


def expected(case, batch=None):
    la = expected_launches(case, batch)
    return ([f.kernel.replace(" ", "") for f in la.fwd], len(la.bwd_data), [w.kernel.replace(" ", "") for w in la.wgrad])


def raw_forward(eng, plan, th, xd, batch, P, C):
    """pyz_mlp_forward into a buffer of max_batch rows per particle filled with a sentinel: (rows written, rows past)."""
    from bayesian_inference_for_nn_amd.engine import _stream, check, ptr
    out = torch.full((P * plan.max_batch * C + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    check(plan.lib.pyz_mlp_forward(plan.h, ptr(th), P, ptr(xd), None, batch, ptr(out), _stream()))
    torch.cuda.synchronize()
    return out[:P * batch * C].view(P, batch, C), out[P * batch * C:]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_dense_case(eng, case, monkeypatch):
    for k in PER_CALL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    spec, P, B = case.spec, case.P, case.batch
    x, y, idx, thetas = case_data(case)
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.max_batch, max_particles=P)
    xd = dev_x(x, case.x_offset)
    yd = dev(y, torch.int32 if spec.loss == "scce" else torch.float32)
    rid = dev(idx, torch.int32) if idx is not None else None
    th = dev(thetas)
    rows, ys = batch_rows(case, x, y, idx)

    if case.sgd:   # k_wgrad_all<1>: the update in the kernel's epilogue; updated parameters against oracle.sgd
        lr = 0.5
        th1, loss1 = dev(thetas[0]), torch.zeros(1, device="cuda")
        with eng.KernelProbe(64) as kp:
            plan.sgd_step(th1, xd, yd, lr, loss1, batch=B, row_idx=rid)
        assert launched(kp) == expected(case), (launched(kp), expected(case), kp.launches)
        st = o_sgd.SGDState(thetas[0])
        rl, _ = o_sgd.sgd_step(st, rows, ys, spec, lr)
        check_loss(loss1.item(), rl, f"{case.name} sgd loss")
        close_blocks(th1, st.theta, spec, what=f"{case.name} sgd theta")
        step = th1.cpu().numpy().astype(np.float64) - thetas[0]     # -lr * gradient, to float32 rounding of theta
        assert np.abs(step - (st.theta - thetas[0])).max() <= 1e-4 * np.abs(st.theta - thetas[0]).max() + \
            2.0 ** -23 * np.abs(thetas[0]).max(), f"{case.name}: sgd step"
        case = case._replace(sgd=False)

    # 1. the launches
    with eng.KernelProbe(64) as kp:
        loss, grad = plan.loss_grad(th, xd, yd, batch=B, row_idx=rid)
    print(case.name, kp.launches)
    assert launched(kp) == expected(case), (launched(kp), expected(case), kp.launches)

    # 2. against the oracle
    out = plan.forward(th, xd, batch=B, row_idx=rid)
    loss_only, none = plan.loss_grad(th, xd, yd, batch=B, row_idx=rid, want_grad=False)
    assert none is None
    assert tuple(out.shape) == (P, B, spec.dims[-1]) and tuple(grad.shape) == (P, spec.n_params)
    loss_h, loss_only_h = loss.cpu().numpy(), loss_only.cpu().numpy()
    for p in check_particles(P):
        rl, rg, rout = o_mlp.loss_and_grad(thetas[p], rows, ys, spec)
        check_loss(loss_h[p], rl, f"{case.name} loss[{p}]")
        check_loss(loss_only_h[p], rl, f"{case.name} loss only[{p}]")
        close_blocks(grad[p], rg, spec, what=f"{case.name} grad[{p}]")
        check_forward(out[p], rout, f"{case.name} forward[{p}]")

    # 4. determinism: fixed combine order, no atomics
    loss2, grad2 = plan.loss_grad(th, xd, yd, batch=B, row_idx=rid)
    assert torch.equal(grad, grad2), f"{case.name}: two gradient calls differ in {int((grad != grad2).sum())} elements"
    assert torch.equal(loss, loss2), f"{case.name}: two loss calls differ"

    # 3. without a gather (rows_cap path): a batch one row shorter on the same plan and the same x
    if idx is None:
        C = spec.dims[-1]
        full, past = raw_forward(eng, plan, th, xd, B, P, C)
        assert torch.equal(full, out), f"{case.name}: forward into a larger buffer differs"
        assert bool((past == SENTINEL).all()), f"{case.name}: forward wrote past its {B} rows"
        if B > 1:
            Bs = B - 1
            out_s = plan.forward(th, xd, batch=Bs)
            loss_s, grad_s = plan.loss_grad(th, xd, yd, batch=Bs)
            assert tuple(out_s.shape) == (P, Bs, C) and tuple(out.shape) == (P, B, C)
            short, past = raw_forward(eng, plan, th, xd, Bs, P, C)
            assert torch.equal(short, out_s)
            assert bool((past == SENTINEL).all()), f"{case.name}: forward wrote past its {Bs} rows"
            rows_s, ys_s = batch_rows(case, x, y, idx, Bs)
            loss_sh = loss_s.cpu().numpy()
            for p in check_particles(P):
                rl, rg, rout = o_mlp.loss_and_grad(thetas[p], rows_s, ys_s, spec)
                check_loss(loss_sh[p], rl, f"{case.name} batch {Bs} loss[{p}]")
                close_blocks(grad_s[p], rg, spec, what=f"{case.name} batch {Bs} grad[{p}]")
                check_forward(out_s[p], rout, f"{case.name} batch {Bs} forward[{p}]")
            fa, fb = expected_launches(case, B, "forward").fwd, expected_launches(case, Bs, "forward").fwd
            if [(f.kernel, f.S) for f in fa] == [(f.kernel, f.S) for f in fb]:   # same summation order per row
                assert torch.equal(out[:, :Bs], out_s), f"{case.name}: forward of the common rows differs between batches"
    plan.close()
