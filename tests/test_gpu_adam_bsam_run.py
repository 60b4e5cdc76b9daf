"""The device-resident ADAM / VADAM / BSAM runs (pyz_adam_run, pyz_bsam_run) against the eager steps they replace, bit
for bit: every epilogue width of the weight-gradient launch (S = 1 / 2 / 4 / 8 / 16 waves), the peeled odd row, gathered
rows, a parameter count that is no multiple of four (the Philox tail), ragged last batches, epoch changes inside a run,
graph replay on and off, chunked and remainder graphs (a graph holds steps of one batch size), inline and uploaded
tables; continuity between runs and eager steps; the fused-perturbation and batch-ahead switches; the float64
restatements; refusals; and quiet train() of the three classes.

Every step of a run is launched for its own batch size, as the eager step is, so the comparison is exact on ragged
batches too (np.array_equal throughout).

The restatement checks keep the tolerance of tests/test_gpu_adam_vadam.py and tests/test_gpu_bsam.py: float32 kernels
against float64, 1e-4 relative to the largest reference magnitude."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from adam_checks import AdamRef, epoch_plan
from bsam_checks import SETTINGS, BsamRef
from oracle import mlp as o_mlp
from oracle import philox as o_philox

from bayesian_inference_for_nn_amd import _lib, synth
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
from bayesian_inference_for_nn_amd.nn import model_from_json, sequential_json
from bayesian_inference_for_nn_amd.optimizers import ADAM, BSAM, VADAM
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (spec, rows, batch): three batches per epoch, the last one ragged (odd but for the one-layer model: 50 = 21 + 21
# + 8).  Waves per workgroup of the weight-gradient launch (pyz_pick_waves, steps = (batch + 1) / 2): 64 -> 4, 23 -> 1;
# 128 -> 8, 45 -> 2; 256 -> 16, 89 -> 4; 21 -> 1, 8 -> 1.  D = 215 and D = 869 are no multiples of four.
MODELS = {
    "scce_s4_s1": (o_mlp.MLPSpec((20, 16, 4), ("relu", "softmax"), "scce"), 151, 64),
    "mse_s8_s2": (o_mlp.MLPSpec((6, 12, 8, 3), ("tanh", "sigmoid", "linear"), "mse"), 301, 128),
    "scce_s16_s4": (o_mlp.MLPSpec((30, 24, 5), ("tanh", "softmax"), "scce"), 601, 256),
    "one_layer_gathered": (o_mlp.MLPSpec((7, 3), ("softmax",), "scce"), 50, 21),
}
KINDS = ("adam", "vadam", "bsam")
COUNTS = (1, 10, 33, 70)          # 33: a graph chunk + a remainder, past the inline tables; 70: two chunks + a remainder
MARKS = (1, 10, 23, 33, 70)       # step counts at which the eager loop's state is kept
LR, B1, B2, LAM, SEED = 0.01, 0.9, 0.999, 0.5, 12345
BSAM_HYP = SETTINGS["sharp"]


def close(gpu, ref, rel=1e-4, what=""):
    gpu = np.asarray(gpu, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(gpu - ref).max()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e})"


@pytest.fixture(scope="module")
def eng(gpu_device):
    from bayesian_inference_for_nn_amd import engine
    return engine


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def make(spec, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, spec.dims[0])).astype(np.float32)
    if spec.loss == "scce":
        y = rng.integers(0, spec.dims[-1], size=n).astype(np.int32)
    else:
        y = rng.normal(size=(n, spec.dims[-1])).astype(np.float32)
    theta = (rng.normal(size=spec.n_params) * 0.3).astype(np.float32)
    return x, y, theta


class Case:
    """One model on the device with the batches of a 70-step loop."""

    def __init__(self, eng, name, epoch0=1, rows=None):
        self.spec, self.n, self.batch = MODELS[name]
        self.n = rows or self.n
        self.x, self.y, self.theta0 = make(self.spec, self.n, seed=sum(map(ord, name)))
        self.plan = eng.MLPPlan(eng.MLPSpec(self.spec.dims, self.spec.acts, self.spec.loss), max_batch=self.batch)
        self.xd = dev(self.x)
        self.yd = dev(self.y, torch.int32 if self.spec.loss == "scce" else torch.float32)
        self.D = self.spec.n_params
        self.batches = [(idx, e + epoch0 - 1) for idx, e in epoch_plan(self.n, self.batch, max(COUNTS), seed=3)]
        self.idx_dev = [dev(idx, torch.int32) for idx, _ in self.batches]

    def state(self, kind, warm=False):
        """theta, m, v at the start: ADAM.py:87-114 (zero moments), BSAM.py:121-141 (m = 0, v = 1) -- or, `warm`, a chain
        that has run before."""
        th = dev(self.theta0)
        if warm:
            rng = np.random.default_rng(17)
            return th, dev(rng.normal(size=self.D) * 0.01), dev(rng.uniform(0.5, 1.5, size=self.D) * (1.0 if kind == "bsam" else 1e-3))
        return th, torch.zeros(self.D, device="cuda"), (torch.ones if kind == "bsam" else torch.zeros)(self.D, device="cuda")

    def table(self, first, count, slot0=0):
        """The (slot0 + count, max_batch) row table and the batch sizes / epochs of steps [first, first + count)."""
        tab = np.zeros((slot0 + count, self.batch), dtype=np.int32)
        for s in range(count):
            idx = self.batches[first + s][0]
            tab[slot0 + s, :len(idx)] = idx
        part = self.batches[first:first + count]
        return dev(tab, torch.int32), [len(i) for i, _ in part], [e for _, e in part]

    def eager(self, kind, state, first, count, step0, losses):
        """`count` eager steps on batches [first, ...): optimizer steps step0 ...; losses[i] / losses[2 i ..] per step."""
        th, m, v = state
        for i in range(count):
            idx, epoch = self.batches[first + i]
            kw = dict(batch=len(idx), row_idx=self.idx_dev[first + i])
            if kind == "bsam":
                self.plan.bsam_step(th, m, v, self.xd, self.yd, num_data=float(self.n), step=step0 + i, seed=SEED,
                                    loss_out=losses[2 * i:2 * i + 2], **BSAM_HYP, **kw)
                continue
            extra = {}
            if kind == "vadam":
                self.plan.vadam_perturb(th, v, LAM, float(self.n), step0 + i, SEED)
                extra = dict(denom_eps=LAM / self.n, decay=LAM / self.n)
            self.plan.adam_step(th, m, v, self.xd, self.yd, LR, B1, B2, epoch, losses[i:i + 1], **extra, **kw)

    def run(self, kind, state, first, count, step0, losses, slot0=0, use_graph=True):
        """The same steps as ONE run, on a stream of its own (graph replay needs one)."""
        th, m, v = state
        tab, sizes, epochs = self.table(first, count, slot0)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            if kind == "bsam":
                self.plan.bsam_run(th, m, v, self.xd, self.yd, tab, sizes, [BSAM_HYP["lr"]] * count, BSAM_HYP["beta_1"],
                                   BSAM_HYP["beta_2"], BSAM_HYP["lam"], BSAM_HYP["rho"], BSAM_HYP["gam"], float(self.n),
                                   step0, SEED, losses, use_graph=use_graph, slot0=slot0)
            else:
                vd = kind == "vadam"
                self.plan.adam_run(th, m, v, self.xd, self.yd, tab, sizes, [LR] * count, epochs, B1, B2, losses,
                                   denom_eps=LAM / self.n if vd else 1e-3, decay=LAM / self.n if vd else 0.0, perturb=vd,
                                   lam=LAM, num_data=float(self.n), step0=step0, seed=SEED, use_graph=use_graph, slot0=slot0)
        stream.synchronize()
        self.plan.check_finite()


def graph_launches(sizes, chunk=32):
    """A graph holds steps of one batch size: chunks of 32 (PYZ_GRAPH_STEPS) inside a stretch of equal batches and one
    graph for the stretch's remainder."""
    n, s = 0, 0
    while s < len(sizes):
        e = s
        while e < len(sizes) and sizes[e] == sizes[s]:
            e += 1
        n += -(-(e - s) // chunk)
        s = e
    return n


def host(state):
    return [t.cpu().numpy() for t in state]


def per_step(kind):
    return 2 if kind == "bsam" else 1


_cases, _eager = {}, {}


def case_of(eng, name):
    if name not in _cases:
        _cases[name] = Case(eng, name)
    return _cases[name]


def eager_marks(eng, name, kind):
    """The eager loop of 70 steps, computed once per (model, kind) and left unchanged: {count: (theta, m, v)}, losses."""
    if (name, kind) not in _eager:
        c = case_of(eng, name)
        st = c.state(kind)
        losses = torch.zeros(per_step(kind) * max(COUNTS), device="cuda")
        marks, done = {}, 0
        for mark in MARKS:
            c.eager(kind, st, done, mark - done, done, losses[per_step(kind) * done:])
            done = mark
            marks[mark] = host(st)
        c.plan.check_finite()
        _eager[(name, kind)] = (marks, losses.cpu().numpy())
    return _eager[(name, kind)]


def assert_same(got_state, got_losses, want_state, want_losses, what):
    for g, w, nm in zip(got_state, want_state, ("theta", "m", "v")):
        assert np.array_equal(g, w), f"{what}: {nm} differs from the eager steps (max {np.abs(g - w).max():.3e})"
    assert np.array_equal(got_losses, want_losses), f"{what}: losses differ (max {np.abs(got_losses - want_losses).max():.3e})"


def test_the_batches_cross_epochs_and_end_ragged(eng):
    for name, (spec, n, batch) in MODELS.items():
        c = case_of(eng, name)
        for count in COUNTS[1:]:
            part = c.batches[:count]
            assert len({e for _, e in part}) - 1 >= 2, "a run must cross at least two epoch boundaries"
            assert any(len(i) < batch for i, _ in part), "... and hold ragged batches"
            if name != "one_layer_gathered":                              # (50 = 21 + 21 + 8)
                assert any(len(i) < batch and len(i) % 2 == 1 for i, _ in part), "... odd ones: the peeled last row"
        epochs = [e for _, e in c.batches]
        for s in range(len(c.batches) - 1):
            if epochs[s + 1] != epochs[s]:
                assert len(c.batches[s][0]) == n % batch < batch, "every epoch ends on its ragged batch"
        assert len(c.batches[32][0]) < batch, "the 33-step run ends on a ragged batch"
    assert MODELS["mse_s8_s2"][0].n_params == 215 and MODELS["scce_s16_s4"][0].n_params == 869


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(MODELS))
def test_run_equals_eager_steps(eng, name, kind, count, use_graph):
    marks, eager_losses = eager_marks(eng, name, kind)
    c, k = case_of(eng, name), per_step(kind)
    st = c.state(kind)
    losses = torch.zeros(k * count, device="cuda")
    c.run(kind, st, 0, count, 0, losses, use_graph=use_graph)
    assert_same(host(st), losses.cpu().numpy(), marks[count], eager_losses[:k * count], f"{name}/{kind}/{count}")
    path, steps = c.plan.last_run_path()
    assert steps == count and path == ("graph" if use_graph else "eager")
    if use_graph:
        assert c.plan.last_run_graph_launches() == graph_launches(c.table(0, count)[1])


@pytest.mark.parametrize("count", [33, 70])
@pytest.mark.parametrize("kind", KINDS)
def test_equal_batches_are_chunked_like_the_other_runs(eng, kind, count):
    """128 rows in batches of 64, no ragged batch: one full graph chunk + a remainder (33, past the inline tables), two
    chunks + a remainder (70, uploaded tables), epochs changing every other step."""
    c, k = Case(eng, "scce_s4_s1", rows=128), per_step(kind)
    assert {len(i) for i, _ in c.batches} == {64} and c.batches[count - 1][1] > 10
    a, b = c.state(kind), c.state(kind)
    la, lb = torch.zeros(k * count, device="cuda"), torch.zeros(k * count, device="cuda")
    c.eager(kind, a, 0, count, 0, la)
    c.run(kind, b, 0, count, 0, lb)
    assert_same(host(b), lb.cpu().numpy(), host(a), la.cpu().numpy(), f"{kind}/{count} equal batches")
    assert c.plan.last_run_path() == ("graph", count) and c.plan.last_run_graph_launches() == -(-count // 32)


@pytest.mark.parametrize("kind", KINDS)
def test_step0_slot0_and_a_later_epoch(eng, kind):
    """The call starts at optimizer step 5 (the Philox step of its first perturbation), loss slot 3 and epoch 4, from a
    chain that has run before."""
    c = Case(eng, "mse_s8_s2", epoch0=4)
    k, count, step0, slot0 = per_step(kind), 10, 5, 3
    a, b = c.state(kind, warm=True), c.state(kind, warm=True)
    la = torch.zeros(k * count, device="cuda")
    lb = torch.full((k * (slot0 + count),), -1.0, device="cuda")
    c.eager(kind, a, 0, count, step0, la)
    c.run(kind, b, 0, count, step0, lb, slot0=slot0)
    lb = lb.cpu().numpy()
    assert_same(host(b), lb[k * slot0:], host(a), la.cpu().numpy(), f"{kind} step0/slot0")
    assert (lb[:k * slot0] == -1.0).all(), "the slots in front of slot0 are not written"
    if kind != "bsam":                                                    # the epoch must matter: epoch 1 gives other weights
        c1 = Case(eng, "mse_s8_s2", epoch0=1)
        other = c1.state(kind, warm=True)
        c1.run(kind, other, 0, count, step0, torch.zeros(count, device="cuda"))
        assert not np.array_equal(host(other)[0], host(b)[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["scce_s4_s1", "one_layer_gathered"])
def test_run_then_steps_then_run_is_the_eager_loop(eng, name, kind):
    """10 steps as a run, 3 eager steps, 10 as a run = 23 eager steps: the last step of a call leaves the weights
    unperturbed, and whoever comes next perturbs them exactly once."""
    marks, eager_losses = eager_marks(eng, name, kind)
    c, k = case_of(eng, name), per_step(kind)
    st = c.state(kind)
    losses = torch.zeros(k * 23, device="cuda")
    c.run(kind, st, 0, 10, 0, losses)
    assert_same(host(st), losses.cpu().numpy()[:k * 10], marks[10], eager_losses[:k * 10], "first run")
    c.eager(kind, st, 10, 3, 10, losses[k * 10:])
    c.run(kind, st, 13, 10, 13, losses, slot0=13)
    assert_same(host(st), losses.cpu().numpy(), marks[23], eager_losses[:k * 23], f"{name}/{kind} run + steps + run")


@pytest.mark.parametrize("kind", KINDS)
def test_a_repeated_call_replays_its_graphs(eng, kind):
    """The same call again (same buffers, same lengths): the same result from the same number of graph launches."""
    c, k, count = Case(eng, "scce_s4_s1"), per_step(kind), 43
    th, m, v = c.state(kind)
    start = [t.clone() for t in (th, m, v)]
    losses = torch.zeros(k * count, device="cuda")
    out = []
    for _ in range(2):
        for t, s in zip((th, m, v), start):
            t.copy_(s)
        c.run(kind, (th, m, v), 0, count, 0, losses)
        assert c.plan.last_run_path() == ("graph", count)
        assert c.plan.last_run_graph_launches() == graph_launches(c.table(0, count)[1])
        # stretches of two full batches and of one ragged batch, on either StepCtl slot, and the one-step remainder
        assert c.plan.adam_run_captures() == (5 if not out else 0), "the second call must replay what the first captured"
        out.append(host((th, m, v)) + [losses.cpu().numpy()])
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    marks, eager_losses = eager_marks(eng, "scce_s4_s1", kind)
    assert np.array_equal(out[0][3][:k * 33], eager_losses[:k * 33])


# ------------------------------------------------------------------ the fused-perturbation switch (read once: a child process)
SWITCH_CASES = [("scce_s4_s1", "vadam"), ("mse_s8_s2", "bsam"), ("scce_s16_s4", "vadam"), ("one_layer_gathered", "bsam"),
                ("mse_s8_s2", "adam")]


def switch_results(eng):
    out = {}
    for name, kind in SWITCH_CASES:
        c = Case(eng, name)
        st = c.state(kind)
        losses = torch.zeros(per_step(kind) * 33, device="cuda")
        c.run(kind, st, 0, 33, 0, losses)
        th, m, v = host(st)
        out.update({f"{name}.{kind}.theta": th, f"{name}.{kind}.m": m, f"{name}.{kind}.v": v,
                    f"{name}.{kind}.losses": losses.cpu().numpy()})
    return out


def child_main(path):
    from bayesian_inference_for_nn_amd import engine
    np.savez(path, **switch_results(engine))


@pytest.mark.parametrize("switch", ["PYZ_ADAM_FUSE_PERTURB", "PYZ_BATCH_AHEAD"])
def test_a_library_switch_at_zero_gives_the_same_bits(eng, tmp_path, switch):
    """PYZ_ADAM_FUSE_PERTURB=0: the perturbation as a launch inside every step of the graph, against the default (in the
    epilogue of the step before).  PYZ_BATCH_AHEAD=0: every step of the multi-layer models gathers its rows like an eager
    step (forward into the contiguous copy, weight gradients from it, no batch assembled ahead) -- the path a model with
    more tiles than spare compute units takes.  Both switches are read once: a child process."""
    assert os.environ.get(switch, "1") != "0"
    path = str(tmp_path / "switched.npz")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_adam_bsam_run as t; t.child_main({path!r})")
    flags = ["-s"] if sys.flags.no_user_site else []
    res = subprocess.run([sys.executable, *flags, "-c", code], env=dict(os.environ, **{switch: "0"}),
                         capture_output=True, text=True, timeout=180)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    theirs, ours = np.load(path), switch_results(eng)
    assert sorted(theirs.files) == sorted(ours)
    for key in ours:
        assert np.array_equal(theirs[key], ours[key]), key
    for name, kind in SWITCH_CASES:                                       # ... and both are the eager loop
        marks, eager_losses = eager_marks(eng, name, kind)
        assert np.array_equal(ours[f"{name}.{kind}.theta"], marks[33][0])
        assert np.array_equal(theirs[f"{name}.{kind}.losses"], eager_losses[:per_step(kind) * 33])


# ------------------------------------------------------------------ against the float64 restatements
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["scce_s4_s1", "mse_s8_s2"])
def test_run_matches_the_float64_restatement(eng, name, kind):
    """Six steps across one epoch change; the perturbations are the oracle's Philox normals of (seed, stream 5 / 6, step)."""
    c, k, count = case_of(eng, name), per_step(kind), 6
    assert len({e for _, e in c.batches[:count]}) == 2
    st = c.state(kind)
    losses = torch.zeros(k * count, device="cuda")
    c.run(kind, st, 0, count, 0, losses)
    ref = BsamRef(c.theta0) if kind == "bsam" else AdamRef(c.theta0)
    want = []
    for i, (idx, epoch) in enumerate(c.batches[:count]):
        if kind == "bsam":
            eps = o_philox.normal(SEED, 6, i, c.D)
            want += list(ref.step(c.x[idx], c.y[idx], c.spec, eps, num_data=float(c.n), **BSAM_HYP))
        elif kind == "vadam":
            ref.perturb(o_philox.normal(SEED, 5, i, c.D), LAM, float(c.n))
            want.append(ref.step(c.x[idx], c.y[idx], c.spec, LR, B1, B2, epoch, denom_eps=LAM / c.n, decay=LAM / c.n))
        else:
            want.append(ref.step(c.x[idx], c.y[idx], c.spec, LR, B1, B2, epoch))
    th, m, v = host(st)
    close(losses.cpu().numpy(), want, what=f"{name}/{kind} losses")
    close(th, ref.theta, what=f"{name}/{kind} theta")
    close(m, ref.m, what=f"{name}/{kind} m")
    close(v, ref.v, what=f"{name}/{kind} v")


# ------------------------------------------------------------------ refusals
def raw_call(c, kind, state, tab, good_sizes, good_epochs, losses, **over):
    """The entry point itself (MLPPlan's own checks would raise first); `over` replaces single arguments."""
    th, m, v = state
    n = len(good_sizes)
    a = dict(plan=c.plan.h, n_steps=n, sizes=good_sizes, epochs=good_epochs, beta_1=B1, beta_2=B2, num_data=float(c.n))
    a.update(over)
    bs = (C.c_int32 * max(n, 1))(*a["sizes"])
    lr = (C.c_float * max(n, 1))(*([LR] * n))
    p = _lib.ptr
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if kind == "bsam":
        return c.plan.lib.pyz_bsam_run(a["plan"], p(th), p(m), p(v), p(c.xd), p(c.yd), p(tab), bs, lr, a["n_steps"], a["beta_1"],
                                       a["beta_2"], 0.5, 0.01, 0.1, a["num_data"], 0, 0, SEED, p(losses), 1, stream)
    ep = (C.c_int64 * max(n, 1))(*a["epochs"])
    return c.plan.lib.pyz_adam_run(a["plan"], p(th), p(m), p(v), p(c.xd), p(c.yd), p(tab), bs, lr, ep, a["n_steps"], a["beta_1"],
                                   a["beta_2"], 1e-3, 0.0, 1 if kind == "vadam" else 0, LAM, a["num_data"], 0, 0, SEED,
                                   p(losses), 1, stream)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_theta_untouched(eng, kind):
    c, k = case_of(eng, "scce_s4_s1"), per_step(kind)
    st = c.state(kind)
    tab, sizes, epochs = c.table(0, 4)
    losses = torch.zeros(k * 4, device="cuda")
    bad = [dict(n_steps=0), dict(sizes=[64, c.batch + 1, 64, 23]), dict(beta_1=1.0), dict(beta_2=1.0)]
    if kind != "bsam":
        bad.append(dict(epochs=[1, 0, 1, 1]))
    if kind != "adam":
        bad.append(dict(num_data=0.0))
    for over in bad:
        rc = raw_call(c, kind, st, tab, sizes, epochs, losses, **over)
        assert rc in (-1, -2), (over, rc)                                 # PYZ_E_INVALID / PYZ_E_SHAPE
        assert c.plan.lib.pyz_last_error()
    # a last layer wider than 32 units: the fused step does not take it
    spec = o_mlp.MLPSpec((12, 20, 40), ("tanh", "softmax"), "scce")
    u = Case.__new__(Case)
    u.spec, u.n, u.batch = spec, 91, 40
    u.x, u.y, u.theta0 = make(spec, 91, seed=2)
    u.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=40)
    u.xd, u.yd, u.D = dev(u.x), dev(u.y, torch.int32), spec.n_params
    u.batches = epoch_plan(91, 40, 4, seed=3)
    ust = u.state(kind)
    utab, usizes, uepochs = u.table(0, 4)
    assert raw_call(u, kind, ust, utab, usizes, uepochs, torch.zeros(k * 4, device="cuda")) == -1
    torch.cuda.synchronize()
    assert np.array_equal(host(st)[0], c.theta0) and np.array_equal(host(ust)[0], u.theta0)
    assert float(losses.abs().max()) == 0.0
    assert raw_call(c, kind, st, tab, sizes, epochs, losses) == 0         # the same call, unspoilt, runs
    torch.cuda.synchronize()
    assert not np.array_equal(host(st)[0], c.theta0)


# ------------------------------------------------------------------ the optimizer classes
def moons_json(classes=2):
    return sequential_json(2, [16, classes], ["relu", "softmax"])


HYPS = {
    ADAM: dict(lr=0.01, beta_1=0.9, beta_2=0.999, batch_size=64),
    VADAM: dict(lr=0.01, beta_1=0.9, beta_2=0.999, batch_size=64),
    BSAM: dict(lr=0.01, beta_1=0.9, beta_2=0.9, lam=0.5, rho=0.01, gam=0.1, batch_size=64),
}


def compiled(cls, classes=2):
    x, y = synth.moons(500, seed=42)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
    cfg = moons_json(classes)
    start = model_from_json(cfg)
    start.reset_glorot(np.random.default_rng(9))
    opt = cls()
    opt.compile(HyperParameters(**HYPS[cls]), cfg, ds, verbose=False, starting_model=start, seed=11)
    return opt


def assert_twins(a, b):
    for t in ("_theta", "_m_dev", "_v_dev", "_running_dev", "_loss_dev"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for t in ("_n", "_epoch_num", "_seen_batches", "_total_batches"):
        assert getattr(a, t) == getattr(b, t), (t, getattr(a, t), getattr(b, t))


@pytest.mark.parametrize("cls", [ADAM, VADAM, BSAM])
def test_quiet_train_is_the_step_loop(cls, gpu_device):
    """train(75) -- resident chunks of 32 and 43 steps, 400 rows in batches of 64: ten epoch changes -- and train(20) on
    top (a run that opens on the old epoch) against step() on a twin."""
    a, b = compiled(cls), compiled(cls)
    for n_it in (75, 20):
        a.train(n_it)
        for _ in range(n_it):
            b.step()
        assert_twins(a, b)
        assert a._plan.last_run_path()[0] == "graph", "the quiet train() must have gone through the run"
        assert a.last_losses.numel() == n_it * (2 if cls is BSAM else 1)
    assert a._n == 95 and a._epoch_num == 14


@pytest.mark.parametrize("cls", [ADAM, VADAM, BSAM])
def test_unfused_model_falls_back_to_the_step_loop(cls, gpu_device):
    """A last layer of 40 units: train() takes the step loop, decided before anything is planned or enqueued."""
    a, b = compiled(cls, classes=40), compiled(cls, classes=40)
    a.train(20)
    for _ in range(20):
        b.step()
    assert_twins(a, b)
    assert not hasattr(a, "last_losses")
