"""Every path of k_dense_fwd_ring against the float64 oracle (tests/ring_cases.py lists the cases and the cells).

Each case first checks the kernel expressions that ran (exactly k_dense_fwd_ring<204, 13, SUB, 8> with the restated SUB
on the ring layer, exactly the fallback kernel where the launch rule refuses), then `forward`, `predict` (the particles
as draws) and `loss_grad` of EVERY particle against oracle.mlp with the Dense matrix's checks, that a second call gives
the same bits, and that the rows past the batch and the words behind the output keep a sentinel.

Isolation: a particle's results do not depend on any other particle's parameters, non-finite included -- every even
particle must give the same bits whether the odd ones are finite, NaN or +Inf.

Forced variants (PYZ_FWD_RING_WAVES / PYZ_FWD_RING_SUB, read once per process): a fresh child process per variant runs
every positive case and the isolation cases, asserts the forced kernel expression and writes its outputs; the parent
compares them bit for bit with the default variant's (every accumulator receives the same matrix instructions in the
same k order whatever SUB and NW are; a zero-padded step adds 0 x 0 to a finite sum)."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ring_cases as rc  # noqa: E402
from head_cases import close_blocks  # noqa: E402
from oracle import mlp as o_mlp  # noqa: E402
from ring_cases import CASES, FORCED, ISOLATION, POSITIVE, fwd_launches  # noqa: E402
from test_gpu_dense_matrix import SENTINEL, check_forward, check_loss, dev, dev_x  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_CALL_ENV = ("PYZ_FWD_LDS", "PYZ_FWD_LDS_MINWG")


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in rc.ENV_FORBIDDEN if os.environ.get(k)]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: every expected launch of this module assumes their "
                    "defaults -- unset them")
    from bayesian_inference_for_nn_amd import engine
    return engine


def device_cus() -> int:
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


@functools.lru_cache(maxsize=None)
def data_of(name):
    return rc.case_data(rc.CASE_BY_NAME[name])


class Dev:
    """A case's plan and inputs on the device."""

    def __init__(self, eng, case):
        self.eng, self.case = eng, case
        spec = case.spec
        x, y, idx, thetas = data_of(case.name)
        self.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.max_batch, max_particles=case.P)
        self.xd = dev_x(x, case.x_offset)
        self.yd = dev(y, torch.int32 if spec.loss == "scce" else torch.float32)
        self.rid = dev(idx, torch.int32) if idx is not None else None
        self.th = dev(thetas)

    def forward(self, th=None):
        with self.eng.KernelProbe(64) as kp:
            out = self.plan.forward(self.th if th is None else th, self.xd, batch=self.case.batch, row_idx=self.rid)
        return out, fwd_names(kp)

    def loss_grad(self, th=None):
        with self.eng.KernelProbe(64) as kp:
            loss, grad = self.plan.loss_grad(self.th if th is None else th, self.xd, self.yd, batch=self.case.batch, row_idx=self.rid)
        return loss, grad, fwd_names(kp)

    def raw_forward(self):
        """pyz_mlp_forward into a buffer of max_batch rows per particle filled with a sentinel: (rows written, rows past)."""
        from bayesian_inference_for_nn_amd.engine import _stream, check, ptr
        P, B, C = self.case.P, self.case.batch, self.case.dims[-1]
        out = torch.full((P * self.case.max_batch * C + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        check(self.plan.lib.pyz_mlp_forward(self.plan.h, ptr(self.th), P, ptr(self.xd), ptr(self.rid), B, ptr(out), _stream()))
        torch.cuda.synchronize()
        return out[:P * B * C].view(P, B, C), out[P * B * C:]

    def close(self):
        self.plan.close()


def fwd_names(kp):
    return [n for n, _ in kp.launches if n.startswith("k_dense_fwd")]


def expected_names(case, call, sub_env=0, nw=8):
    return [f.kernel for f in fwd_launches(case, call, device_cus(), sub_env, nw)]


def set_env(monkeypatch, case):
    for k in PER_CALL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------- every case against the oracle
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_ring_case(eng, case, monkeypatch):
    set_env(monkeypatch, case)
    spec, P, B = case.spec, case.P, case.batch
    x, y, idx, thetas = data_of(case.name)
    rows, ys = rc.batch_rows(case, x, y, idx)
    d = Dev(eng, case)

    # 1. the kernel expressions that ran
    out, names_f = d.forward()
    loss, grad, names_g = d.loss_grad()
    print(case.name, names_f, names_g)
    assert names_f == expected_names(case, "forward"), (names_f, expected_names(case, "forward"))
    assert names_g == expected_names(case, "grad"), (names_g, expected_names(case, "grad"))

    # 2. forward, predict, loss and gradient of every particle
    assert tuple(out.shape) == (P, B, spec.dims[-1]) and tuple(grad.shape) == (P, spec.n_params)
    samples = None
    if idx is None:
        with eng.KernelProbe(64) as kp:
            samples, _ = d.plan.predict(d.th, d.xd)
        assert fwd_names(kp) == expected_names(case, "forward"), kp.launches
        assert tuple(samples.shape) == tuple(out.shape)
    loss_h = loss.cpu().numpy()
    for p in range(P):
        rl, rg, rout = o_mlp.loss_and_grad(thetas[p], rows, ys, spec)
        check_forward(out[p], rout, f"{case.name} forward[{p}]")
        if samples is not None:
            check_forward(samples[p], rout, f"{case.name} predict[{p}]")
        check_loss(loss_h[p], rl, f"{case.name} loss[{p}]")
        close_blocks(grad[p], rg, spec, what=f"{case.name} grad[{p}]")   # (gathered: through the batch copy the forward left)

    # 3. determinism: a second call gives the same bits (gathered: the batch copy is the same again)
    out2, _ = d.forward()
    loss2, grad2, _ = d.loss_grad()
    assert torch.equal(out, out2), f"{case.name}: two forward calls differ in {int((out != out2).sum())} elements"
    assert torch.equal(grad, grad2), f"{case.name}: two gradient calls differ in {int((grad != grad2).sum())} elements"
    assert torch.equal(loss, loss2), f"{case.name}: two loss calls differ"

    # 4. nothing else written
    full, past = d.raw_forward()
    assert torch.equal(full, out), f"{case.name}: forward into a larger buffer differs"
    assert bool((past == SENTINEL).all()), f"{case.name}: forward wrote past its {B} rows"
    d.close()


# ---------------------------------------------------------------- isolation
def first_difference(a, b):
    ne = (a != b) | (torch.isnan(a) != torch.isnan(b))
    ne &= ~(torch.isnan(a) & torch.isnan(b))
    if not bool(ne.any()):
        return None
    at = tuple(int(i) for i in ne.nonzero()[0])
    return at, float(a[at]), float(b[at]), int(ne.sum())


def check_isolation(d, what):
    """Every even particle: the same bits with the odd particles finite, NaN and +Inf (no tolerance, no excluded element);
    and the finite call again afterwards (nothing non-finite stays behind in the workspace)."""
    case = d.case
    assert case.P % 2 == 0
    out0, _ = d.forward()
    loss0, grad0, _ = d.loss_grad()
    assert bool(torch.isfinite(out0).all()) and bool(torch.isfinite(grad0).all()) and bool(torch.isfinite(loss0).all())
    for label, bad in (("NaN", float("nan")), ("+Inf", float("inf"))):
        th = d.th.clone()
        th[1::2] = bad
        out, _ = d.forward(th)
        loss, grad, _ = d.loss_grad(th)
        for name, got, want in (("forward", out, out0), ("loss", loss, loss0), ("gradient", grad, grad0)):
            diff = first_difference(got[0::2], want[0::2])
            if diff is not None:
                at, g, w, n = diff
                pytest.fail(f"{what}: odd particles {label}: {name} of even particle {2 * at[0]} differs at {at[1:]}: "
                            f"{g!r} instead of {w!r} ({n} elements of the even particles differ)")
    out, _ = d.forward()
    loss, grad, _ = d.loss_grad()
    assert torch.equal(out, out0) and torch.equal(loss, loss0) and torch.equal(grad, grad0), f"{what}: the finite call differs afterwards"


@pytest.mark.parametrize("case", ISOLATION, ids=[c.name for c in ISOLATION])
def test_particles_do_not_read_each_other(eng, case, monkeypatch):
    """Before its buffer range ended at &W[K][0], the ring's last slab read on into the bias row, the following layers
    and the NEXT particle's first weights (K % KS != 0) and multiplied them by the zeros staged for A: 0 x Inf = NaN.
    On that library s2_k20_ns1_iso failed here with
        odd particles NaN: forward of even particle 0 differs at (0, 0): nan instead of 0.7994316816329956
        (9312 elements of the even particles differ)
    -- all 32 x 97 x 3 outputs of the even particles -- and s1_k20_ns2_iso likewise (15456 = 32 x 161 x 3 elements);
    the case with K % KS == 0 and the two fallback kernels passed."""
    set_env(monkeypatch, case)
    names = expected_names(case, "forward")
    d = Dev(eng, case)
    _, got = d.forward()
    assert got == names, (got, names)
    check_isolation(d, case.name)
    d.close()


# ---------------------------------------------------------------- the forced variants (read once: a child process)
_default = {}
_stopped = []     # why no further child is started


def variant_results(eng, sub_env=0, nw=8):
    """forward, loss and gradient of every positive case, with the ring's kernel expression asserted."""
    res = {}
    for case in POSITIVE:
        d = Dev(eng, case)
        out, names_f = d.forward()
        loss, grad, names_g = d.loss_grad()
        for call, names in (("forward", names_f), ("grad", names_g)):
            assert names == expected_names(case, call, sub_env, nw), (case.name, call, names)
        res[f"{case.name}.out"], res[f"{case.name}.loss"], res[f"{case.name}.grad"] = (t.cpu().numpy() for t in (out, loss, grad))
        if case.isolate:
            check_isolation(d, f"{case.name} (SUB {sub_env}, {nw} waves)")
        d.close()
    return res


def default_results(eng):
    if not _default:
        _default.update(variant_results(eng))
    return _default


def child_main(path, sub, nw):
    from bayesian_inference_for_nn_amd import engine
    assert os.environ.get("PYZ_FWD_RING_SUB") == str(sub) and os.environ.get("PYZ_FWD_RING_WAVES", "8") == str(nw)
    np.savez(path, **variant_results(engine, sub, nw))


@pytest.mark.parametrize("name,env,sub,nw", FORCED, ids=[f[0] for f in FORCED])
def test_a_forced_variant_gives_the_same_bits(eng, tmp_path, name, env, sub, nw):
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    path = str(tmp_path / "forced.npz")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_ring_matrix as t; t.child_main({path!r}, {sub}, {nw})")
    flags = ["-s"] if sys.flags.no_user_site else []
    try:
        res = subprocess.run([sys.executable, *flags, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                             timeout=120)
    except subprocess.TimeoutExpired:
        _stopped.append(f"the child of {name} ran into its time limit")
        raise
    if res.returncode < 0 or res.returncode in (124, 134, 137, 139):
        _stopped.append(f"the child of {name} ended with status {res.returncode}")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    theirs, ours = np.load(path), default_results(eng)
    assert sorted(theirs.files) == sorted(ours)
    for key in sorted(ours):
        a, b = torch.as_tensor(theirs[key]), torch.as_tensor(ours[key])
        assert torch.equal(a, b), f"{name}: {key} differs from the default variant in {int((a != b).sum())} elements " \
                                  f"(max |diff| {float((a - b).abs().max()):.3e})"
