"""pyz_lane_scores on the device: every lane's loss sum and wrong rows on a data split against the float64 oracle and against
pyz_mlp_loss_grad, for the SCCE, MSE and BCE cases of tests/sgld_chains_checks.py at their starting rows and batch rows.

Losses: 1e-4 relative, the project's bound on a loss.  Error counts: exactly the oracle's -- which holds because no row of
any lane is a near-tie: the oracle's top-two output gap (SCCE) or |p - 0.5| (BCE) is at least 1e-4 everywhere, asserted
here on the CPU side for every lane and row (float32 outputs of these small nets are good to about 1e-6)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bce_checks  # noqa: E402
import sgld_chains_checks as cc  # noqa: E402
from oracle import mlp as o_mlp  # noqa: E402

GAP = 1e-4
REL = 1e-4


@pytest.fixture(scope="module")
def eng(gpu_device):
    from bayesian_inference_for_nn_amd import engine
    return engine


@pytest.fixture(autouse=True)
def bce(monkeypatch):
    bce_checks.install(monkeypatch)          # the oracle restated for the BCE case of the list


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


_REFS = {}


def reference(spec, thetas, rows, ys):
    """Per lane, in float64: (mean loss, wrong rows), with the no-near-tie condition asserted for every row."""
    losses, wrong = [], []
    y = np.asarray(ys)
    for c, theta in enumerate(np.asarray(thetas, dtype=np.float64)):
        loss, _, out = o_mlp.loss_and_grad(theta, rows, ys, spec, np.float64)
        losses.append(float(loss))
        if spec.loss == "scce":
            top = np.sort(out, axis=1)
            gap = top[:, -1] - top[:, -2]
            assert gap.min() >= GAP, f"lane {c}: a row's top two outputs are {gap.min():.3e} apart"
            wrong.append(int((np.argmax(out, axis=1) != y.reshape(-1)).sum()))
        elif spec.loss == "bce":
            p = out.reshape(-1)
            assert np.abs(p - 0.5).min() >= GAP, f"lane {c}: a row's p is {np.abs(p - 0.5).min():.3e} from 0.5"
            wrong.append(int(((p > 0.5) != (y.reshape(-1) > 0.5)).sum()))
        else:
            wrong.append(0)
    return np.array(losses), np.array(wrong, dtype=np.int64)


def case_reference(case):
    if case.name not in _REFS:                # computed once, shared, never written to
        data = cc.chains_data(case)
        ref = reference(case.step.spec, data.theta0, data.step.rows, data.step.ys)
        for a in ref:
            a.setflags(write=False)
        _REFS[case.name] = (data, ref)
    return _REFS[case.name]


def device_inputs(case, data, pad=0, fill=np.nan):
    """x, y of the batch rows on the device; pad > 0: views of buffers with `pad` rows of `fill` behind them."""
    spec = case.step.spec
    rows = np.asarray(data.step.rows, dtype=np.float32)
    ys = np.asarray(data.step.ys)
    n = len(rows)
    ydt = torch.int32 if spec.loss == "scce" else torch.float32
    ys = ys.reshape(n) if spec.loss == "scce" else ys.reshape(n, -1)
    if not pad:
        return dev(rows), dev(ys, ydt)
    xb = np.concatenate([rows, np.full((pad, rows.shape[1]), fill, dtype=np.float32)])
    yfill = np.full((pad,) + ys.shape[1:], 7 if spec.loss == "scce" else fill, dtype=ys.dtype)
    yb = np.concatenate([ys, yfill])
    return dev(xb)[:n], dev(yb, ydt)[:n]


def check_against(case, ref, loss_sum, errors, n, what):
    ref_loss, ref_wrong = ref
    got = loss_sum.cpu().numpy() / n
    assert got.dtype == np.float64 and got.shape == ref_loss.shape
    rel = np.abs(got - ref_loss) / np.abs(ref_loss)
    print(f"SCORES | {case.name} | {what} | loss error / bound {rel.max() / REL:.4f} | wrong rows {ref_wrong.tolist()} of {n}")
    assert np.all(rel <= REL), f"{case.name} {what}: loss {got} against {ref_loss}"
    if errors is not None:
        e = errors.cpu().numpy()
        assert e.dtype == np.int64 and np.array_equal(e, ref_wrong), f"{case.name} {what}: wrong rows {e} against {ref_wrong}"


@pytest.mark.parametrize("case", cc.CASES, ids=[c.name for c in cc.CASES])
def test_lane_scores_case(eng, case):
    data, ref = case_reference(case)
    spec, st = case.step.spec, case.step
    n = len(data.step.rows)
    assert n == st.batch
    weights = dev(data.theta0)
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=st.max_batch, max_particles=case.P)
    x, y = device_inputs(case, data)
    loss_sum, errors = plan.lane_scores(weights, x, y)
    check_against(case, ref, loss_sum, errors, n, "P lanes")
    # ... and pyz_mlp_loss_grad's per-particle loss on the same rows
    lg, _ = plan.loss_grad(weights, x, y, want_grad=False)
    lg = lg.cpu().numpy().astype(np.float64)
    got = loss_sum.cpu().numpy() / n
    assert np.all(np.abs(got - lg) <= REL * np.abs(lg)), f"{case.name}: {got} against loss_grad's {lg}"
    # the same call twice: the same bits
    again, errors2 = plan.lane_scores(weights, x, y)
    assert torch.equal(again.view(torch.int64), loss_sum.view(torch.int64)) and torch.equal(errors, errors2)
    # n < max_batch, NaN in the rows beyond n (and labels outside the classes): never read, the same bits
    assert n < plan.max_batch
    xp, yp = device_inputs(case, data, pad=plan.max_batch - n)
    padded, errors3 = plan.lane_scores(weights, xp, yp)
    assert torch.equal(padded.view(torch.int64), loss_sum.view(torch.int64)) and torch.equal(errors, errors3)
    # no error counts asked
    only, none = plan.lane_scores(weights, x, y, want_errors=False)
    assert none is None and torch.equal(only.view(torch.int64), loss_sum.view(torch.int64))
    plan.close()
    if case.P > 2:                            # more lanes than max_particles: chunks of 2, 2, 1
        small = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=st.max_batch, max_particles=2)
        loss_sum, errors = small.lane_scores(weights, x, y)
        check_against(case, ref, loss_sum, errors, n, "chunks of 2")
        small.close()


@pytest.mark.parametrize("loss", ("scce", "mse", "bce"))
def test_more_than_one_workgroup_per_lane(eng, loss):
    """600 rows = three workgroups of 256 rows per lane (the cases above have one): the partials of a lane are added in
    workgroup order by whichever workgroup finishes last, so ten calls give one set of bits."""
    dims, acts = {"scce": ((6, 9, 4), ("tanh", "softmax")), "mse": ((6, 9, 3), ("tanh", "linear")),
                  "bce": ((6, 9, 1), ("tanh", "sigmoid"))}[loss]
    spec = bce_checks.spec(dims, acts) if loss == "bce" else o_mlp.MLPSpec(dims, acts, loss)
    rng = np.random.default_rng(41)
    n, P = 600, 3
    rows = rng.normal(size=(n, dims[0])).astype(np.float32)
    thetas = (rng.normal(size=(P, spec.n_params)) * 0.7).astype(np.float32)
    if loss == "scce":
        ys = rng.integers(0, dims[-1], size=n).astype(np.int32)
    elif loss == "mse":
        ys = rng.normal(size=(n, dims[-1])).astype(np.float32)
    else:
        ys = (rng.uniform(size=(n, 1)) > 0.5).astype(np.float32)
    # rows whose decision is a near-tie for any lane leave the data (the condition of the exact error count)
    keep = np.ones(n, dtype=bool)
    for theta in thetas.astype(np.float64):
        out = o_mlp.loss_and_grad(theta, rows, ys, spec, np.float64)[2]
        if loss == "scce":
            top = np.sort(out, axis=1)
            keep &= (top[:, -1] - top[:, -2]) >= GAP
        elif loss == "bce":
            keep &= np.abs(out.reshape(-1) - 0.5) >= GAP
    rows, ys = rows[keep], ys[keep]
    n = len(rows)
    assert n > 512
    ref = reference(spec, thetas, rows, ys)
    plan = eng.MLPPlan(eng.MLPSpec(dims, acts, loss), max_batch=n, max_particles=P)
    x, y, w = dev(rows), dev(ys, torch.int32 if loss == "scce" else torch.float32), dev(thetas)
    first, errors = plan.lane_scores(w, x, y)
    got = first.cpu().numpy() / n
    assert np.all(np.abs(got - ref[0]) <= REL * np.abs(ref[0])), (got, ref[0])
    assert np.array_equal(errors.cpu().numpy(), ref[1])
    if loss != "mse":
        assert 0 < ref[1].min() and ref[1].max() < n
    for _ in range(9):
        again, e2 = plan.lane_scores(w, x, y)
        assert torch.equal(again.view(torch.int64), first.view(torch.int64)) and torch.equal(e2, errors)
    plan.close()


def test_argument_errors(eng):
    from bayesian_inference_for_nn_amd._lib import ptr
    spec = eng.MLPSpec((3, 4, 2), ("tanh", "softmax"), "scce")
    plan = eng.MLPPlan(spec, max_batch=8, max_particles=2)
    w = torch.zeros((2, spec.n_params), device="cuda")
    x, y = torch.zeros((9, 3), device="cuda"), torch.zeros(9, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert plan.lib.pyz_lane_scores(plan.h, ptr(w), 2, ptr(x), ptr(y), 9, ptr(out), None, None) == -2      # n > max_batch
    for args in ((None, 2, ptr(x), ptr(y), 8, ptr(out)), (ptr(w), 0, ptr(x), ptr(y), 8, ptr(out)),
                 (ptr(w), 2, None, ptr(y), 8, ptr(out)), (ptr(w), 2, ptr(x), None, 8, ptr(out)),
                 (ptr(w), 2, ptr(x), ptr(y), 0, ptr(out)), (ptr(w), 2, ptr(x), ptr(y), 8, None)):
        assert plan.lib.pyz_lane_scores(plan.h, *args, None, None) == -1
    with pytest.raises(ValueError):
        plan.lane_scores(w, x, y)                         # nine rows for a plan of eight
    with pytest.raises(ValueError):
        plan.lane_scores(w[:, :-1].contiguous(), x[:8], y[:8])
    plan.close()
