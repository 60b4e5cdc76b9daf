"""Every device-resident SGD, SWAG, SGLD and BBB run path (pyz_sgd_run, pyz_swag_run, pyz_sgld_run, pyz_bbb_run: all four are
sgld_run_impl over the shared upload_run_tables and PyzGraphCache) against the float64 oracle and against the eager steps (tests/run_cases.py lists the cases and cells).

Oracle tier: a short ragged run of six steps, launched for its largest batch while later steps have 1, an odd number or fewer
than 2 S rows.  Every prefix of it runs from the same start, so the state after prefix i is the state before step i and
every step is compared on its own with the float64 reference restarted from that state (run_cases.compare_run_step, i.e.
step_cases.compare_step unchanged), with the device's own Philox noise.  The full run replayed from graphs must give the
bits of the eager-chained one, twice.  Losses and costs land in slot slot0 + i only; sentinels stand around every state
vector, the loss / cost / validation arrays, the deviation matrix and the row table, whose entries behind a step's batch are
other valid rows.
Chain tier: runs of 32, 33 and 70 steps and a second call that continues count and slots, against the same steps as eager
*_step calls: bit for bit with whole batches, 2e-6 of the largest magnitude with a ragged last batch per epoch (the launch
geometry differs there: tests/test_gpu_batch_ahead.py).
Then: the launches of a run, the SWAG and BBB bookkeeping cells, the graph cache and the per-run tables, the run-wide
switches in child processes, and pyz_check_finite after a diverged run.

Not covered: growth of the device tables past 65 536 steps and of the pinned staging buffers past 4096 steps."""

import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import run_cases as rc  # noqa: E402
from run_cases import BOOKS, CASES, FUSED_CASES, UNFUSED_CASES, RunCall, compare_run_step, ref_run_step  # noqa: E402
from test_gpu_step_matrix import SENTINEL, TAIL, Guarded, dev  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -7.0          # what the loss, cost and validation slots hold before a run
WORST = {}           # mode -> (largest error / tolerance, case, step, quantity): printed at the end of the module
E_INVALID = -1       # PYZ_E_INVALID
_DATA = {}


def data_of(case):
    if case.name not in _DATA:
        _DATA[case.name] = rc.run_data(case, slots=140)
    return _DATA[case.name]


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in rc.ENV_FORBIDDEN if os.environ.get(k)]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the library reads them once per process and every "
                    "expected launch and graph of this module assumes their defaults -- unset them")
    from bayesian_inference_for_nn_amd import engine
    yield engine
    for mode, (ratio, name, step, q) in sorted(WORST.items()):
        print(f"WORST | {mode} | error / tolerance {ratio:.4f} | {name} | step {step} | {q}")


class Block:
    """An array of any shape as a view into a sentinel-filled buffer (four elements in front, 64 behind)."""

    def __init__(self, values, dtype=torch.float32, sentinel=SENTINEL):
        values = np.ascontiguousarray(values)
        self.sentinel, self.n = sentinel, values.size
        self.buf = torch.full((4 + self.n + TAIL,), sentinel, dtype=dtype, device="cuda")
        self.t = self.buf[4:4 + self.n].view(values.shape)
        self.t.copy_(dev(values, dtype))
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    def set(self, values):
        self.t.copy_(dev(values, self.t.dtype))

    def get(self):
        return self.t.cpu().numpy().copy()

    def intact(self):
        return bool((self.buf[:4] == self.sentinel).all()) and bool((self.buf[4 + self.n:] == self.sentinel).all())


def prefix(call: RunCall, p: int) -> RunCall:
    return call._replace(sizes=call.sizes[:p], lrs=call.lrs[:p])


def after(call: RunCall, sizes, lrs) -> RunCall:
    """The call that continues `call`: its count and slots go on."""
    return call._replace(n0=call.n0 + len(call.sizes), slot0=call.slot0 + len(call.sizes), sizes=tuple(sizes), lrs=tuple(lrs))


class Dev:
    """The device side of one (case, mode): plan, data, guarded buffers; `run` is one call of the mode's run entry point,
    `eager` the same steps as single *_step calls."""

    def __init__(self, eng, case, mode, data, slots=80, val=False):
        self.eng, self.case, self.mode, self.data, self.slots = eng, case, mode, data, slots
        spec, d = case.spec, data.step
        self.espec = eng.MLPSpec(spec.dims, spec.acts, spec.loss)
        self.plan = eng.MLPPlan(self.espec, max_batch=case.max_batch)
        ydt = torch.int32 if spec.loss == "scce" else torch.float32
        self.x, self.y = dev(d.x), dev(d.y, ydt)
        self.tab = Block(data.tab[:slots], torch.int32, sentinel=1)      # (a sentinel that is itself a valid row)
        self.bufs = {}
        self.pm = Guarded(d.pm_vec, case.aligned) if case.prior_vec else None
        self.pr = Guarded(d.pr_vec, case.aligned) if case.prior_vec else None
        self.out = Block(np.full((slots, 4) if mode == "bbb" else (slots,), FILL, np.float32))
        self.vals = Block(np.full((slots,), FILL, np.float32))
        self.vplan = None
        if val:
            self.vplan = eng.MLPPlan(self.espec, max_batch=rc.VAL_MAX_BATCH)
            self.xv, self.yv = dev(data.xv), dev(data.yv, ydt)
        self.seed, self.alpha, self.prior = case.seed, case.step.alpha, case.step.prior
        self.one = torch.zeros(4, device="cuda")

    def close(self):
        self.plan.close()
        if self.vplan is not None:
            self.vplan.close()

    # ---- state
    def reset(self, s, fill=True):
        for key, v in s.items():
            if key == "dev":
                if "dev" not in self.bufs or tuple(self.bufs["dev"].t.shape) != v.shape:
                    self.bufs["dev"] = Block(v)
                self.bufs["dev"].set(v)
            elif key not in self.bufs:
                self.bufs[key] = Guarded(v, self.case.aligned)
            else:
                self.bufs[key].set(v)
        if fill:
            self.out.t.fill_(FILL)
            self.vals.t.fill_(FILL)

    def state(self):
        torch.cuda.synchronize()
        return {key: b.get().reshape(b.t.shape) for key, b in self.bufs.items()}

    def outputs(self):
        torch.cuda.synchronize()
        return self.out.get(), self.vals.get()

    def guards(self):
        named = list(self.bufs.items()) + [("pm", self.pm), ("pr", self.pr), ("losses", self.out), ("val_losses", self.vals),
                                            ("row table", self.tab)]
        return [key for key, b in named if b is not None and not b.intact()]

    # ---- one call of the run entry point
    def run(self, call, use_graph=True, side=True):
        b, p = self.bufs, self.plan
        kw = dict(use_graph=use_graph, slot0=call.slot0)

        def go():
            if self.mode == "sgd":
                p.sgd_run(b["theta"].t, self.x, self.y, self.tab.t, call.sizes, call.lrs, self.out.t, **kw)
            elif self.mode == "swag":
                p.swag_run(b["theta"].t, b["mean"].t, b["sq"].t, b["dev"].t, call.freq, self.x, self.y, self.tab.t, call.sizes,
                           call.lrs, call.n0, self.out.t, **kw)
            elif self.mode == "sgld":
                p.sgld_run(b["theta"].t, b["mean"].t, b["sq"].t, self.x, self.y, self.tab.t, call.sizes, call.lrs, call.n0,
                           self.seed, self.out.t, **kw)
            else:
                v = self.vplan if call.val else None
                p.bbb_run(b["mu"].t, b["rho"].t, b["w"].t, self.x, self.y, self.tab.t, call.sizes, call.lrs, self.alpha,
                          self.prior[0], self.prior[1], call.n0, self.seed, self.out.t,
                          prior_mean_vec=self.pm.t if self.pm else None, prior_rho_vec=self.pr.t if self.pr else None,
                          val_plan=v, val_x=self.xv if v else None, val_y=self.yv if v else None,
                          val_losses_out=self.vals.t if v else None, **kw)

        if not side:
            go()
            return
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            go()
        st.synchronize()

    def run_on(self, stream, call, use_graph=True):
        """The call on a stream of the caller's, without synchronising."""
        with torch.cuda.stream(stream):
            self.run(call, use_graph, side=False)

    # ---- the same steps as eager *_step calls
    def eager(self, call):
        b, p, one = self.bufs, self.plan, self.one
        for i, (size, lr) in enumerate(zip(call.sizes, call.lrs)):
            n, slot = call.n0 + i, call.slot0 + i
            kw = dict(batch=size, row_idx=self.tab.t[slot, :size])
            if self.mode == "sgd":
                p.sgd_step(b["theta"].t, self.x, self.y, lr, one[:1], **kw)
            elif self.mode == "swag":
                hit = n % call.freq == 0
                row = b["dev"].t[rc.swag_row(n, call.k, call.freq)] if hit else None
                p.swag_step(b["theta"].t, b["mean"].t, b["sq"].t, row, self.x, self.y, lr, n, hit, one[:1], **kw)
            elif self.mode == "sgld":
                p.sgld_step(b["theta"].t, b["mean"].t, b["sq"].t, self.x, self.y, lr, n, self.seed, one[:1], **kw)
            else:
                p.bbb_step(b["mu"].t, b["rho"].t, b["w"].t, self.x, self.y, lr, self.alpha, self.prior[0], self.prior[1], n,
                           self.seed, one, prior_mean_vec=self.pm.t if self.pm else None,
                           prior_rho_vec=self.pr.t if self.pr else None, **kw)
                self.out.t[slot, :3] = one[:3]
                if call.val and n % rc.GATE_MOD:
                    vl, _ = self.vplan.loss_grad(b["w"].t, self.xv, self.yv, want_grad=False)
                    self.vals.t[slot] = vl[0]
                continue
            self.out.t[slot] = one[0]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def assert_same(got, want, what, exact=True):
    """(state, (losses, vals)) against (state, (losses, vals)): bit for bit, or 2e-6 of the largest magnitude."""
    (gs, go), (ws, wo) = got, want
    pairs = [(k, gs[k], ws[k]) for k in ws] + [("losses", go[0], wo[0]), ("validation losses", go[1], wo[1])]
    for name, a, b in pairs:
        if exact:
            assert same_bits(a, b), f"{what}: {name} differs (max {np.abs(a.astype(np.float64) - b).max():.3e})"
        else:
            scale = max(float(np.abs(b).max()), 1e-30)
            err = float(np.abs(a.astype(np.float64) - b).max())
            assert err <= 2e-6 * scale, f"{what}: {name}: {err:.3e} vs scale {scale:.3e}"


def written_slots(case, mode, out):
    """The slots of the loss / cost array a run wrote; every other entry, and the fourth cost column, still hold FILL."""
    if mode == "bbb":
        assert np.all(out[:, 3] == FILL), "the fourth cost column was written"
        rows = np.flatnonzero(np.any(out[:, :3] != FILL, axis=1))
        assert np.all(out[rows, :3] != FILL)
        return list(rows)
    return list(np.flatnonzero(out != FILL))


def note(mode, case, i, rep):
    for q, r in sorted(rep.items()):
        print(f"{case.name} {mode} step {i}: {q}: error / tolerance {r:.4f}")
        if r > WORST.get(mode, (-1.0,))[0]:
            WORST[mode] = (r, case.name, i, q)


def per_step(d, case, data, call, mode, start, what):
    """The oracle tier's method on one call from the state `start`: every prefix eager-chained, the full call from graphs
    twice, every step against the float64 reference restarted from the state before it.  Returns the final state."""
    n = len(call.sizes)
    states, outs = [start], []
    for p in range(1, n + 1):
        d.reset(start)
        d.run(prefix(call, p), use_graph=False, side=False)
        assert d.plan.last_run_path() == ("eager", p) and d.plan.last_run_graph_launches() == 0
        states.append(d.state())
        outs.append(d.outputs())
        assert d.guards() == [], f"{what}: prefix {p} wrote outside {d.guards()}"
        assert written_slots(case, mode, outs[-1][0]) == list(range(call.slot0, call.slot0 + p)), f"{what}: prefix {p}: slots written"
        if p > 1:
            k = call.slot0 + p - 1
            assert same_bits(outs[-1][0][:k], outs[-2][0][:k]), f"{what}: prefix {p} gives its first {p - 1} losses other bits"
            assert same_bits(outs[-1][1][:k], outs[-2][1][:k]), f"{what}: prefix {p}: validation losses of the first {p - 1} steps"
    for rep in range(2):
        d.reset(start)
        d.run(call, use_graph=True, side=True)
        assert (d.plan.last_run_path(), d.plan.last_run_graph_launches()) == rc.expected_run_path(n, True, True)
        assert_same((d.state(), d.outputs()), (states[-1], outs[-1]), f"{what}: graph run {rep} against the eager-chained run")
        assert d.guards() == []
    for i in range(n):
        s0 = states[i]
        ref = ref_run_step(case, data, call, mode, i, s0)
        got = dict(states[i + 1])
        out, vals = outs[i]
        slot = written_slots(case, mode, out)[-1]
        got["slot"] = slot
        if mode == "bbb":
            got["cost"] = out[slot, :3]
            if call.val:
                assert set(np.flatnonzero(vals != FILL)) <= set(range(call.slot0, call.slot0 + i + 1))
                got["val"] = None if vals[slot] == FILL else vals[slot]
        else:
            got["loss"] = out[slot]
        note(mode, case, i, compare_run_step(case, data, call, mode, i, s0, got, ref, what=f"{what}: "))
    return states[-1]


# ---------------------------------------------------------------- oracle tier
PAIRS = [(c, m) for c in CASES for m in c.modes]
PAIR_IDS = [f"{c.name}-{m}" for c, m in PAIRS]


@pytest.mark.parametrize("case,mode", PAIRS, ids=PAIR_IDS)
def test_every_step_of_a_ragged_run(eng, case, mode):
    data = data_of(case)
    call = case.call(mode)
    d = Dev(eng, case, mode, data)
    per_step(d, case, data, call, mode, rc.initial_state(mode, data, call.k), f"{case.name} {mode}")
    d.plan.check_finite()
    d.close()


# ---------------------------------------------------------------- chain tier
def chain_calls(case, mode, n, ragged, val=False):
    """n steps and five more as a second call; learning rates a 64th of the case's (a long chain at the step tests' rate
    would amplify the summation-order difference of a ragged batch past any fixed bound), changing with every step."""
    lr = (case.bbb_lr if mode == "bbb" else case.lr) / 64
    small = case.sizes[1]
    sizes = [small if (ragged and i % 3 == 2) else case.bmax for i in range(n + 5)]
    lrs = [lr * (1.0 - (i % 8) / 16.0) for i in range(n + 5)]
    k, freq = case.swag if mode == "swag" else (0, 0)
    first = RunCall(case.n0, case.slot0, tuple(sizes[:n]), tuple(lrs[:n]), k, freq, val)
    return first, after(first, sizes[n:], lrs[n:])


def chain(eng, case, mode, n, ragged):
    data = data_of(case)
    val = mode == "bbb"
    first, second = chain_calls(case, mode, n, ragged, val)
    d = Dev(eng, case, mode, data, val=val)
    start = rc.initial_state(mode, data, first.k)
    d.reset(start)
    d.eager(first)
    d.eager(second)
    want = (d.state(), d.outputs())
    for use_graph in (True, False):
        d.reset(start)
        d.run(first, use_graph=use_graph)
        assert (d.plan.last_run_path(), d.plan.last_run_graph_launches()) == rc.expected_run_path(n, use_graph, True)
        d.run(second, use_graph=use_graph)
        assert (d.plan.last_run_path(), d.plan.last_run_graph_launches()) == rc.expected_run_path(5, use_graph, True)
        got = (d.state(), d.outputs())
        assert_same(got, want, f"{case.name} {mode} {n}+5 steps, graphs {use_graph}", exact=not ragged)
        assert written_slots(case, mode, got[1][0]) == list(range(case.slot0, case.slot0 + n + 5))
        assert d.guards() == []
    d.plan.check_finite()
    d.close()


FUSED_PAIRS = [(c, m) for c in FUSED_CASES for m in c.modes]


@pytest.mark.parametrize("ragged", [False, True], ids=["whole", "ragged"])
@pytest.mark.parametrize("n", rc.CHAIN_COUNTS)
@pytest.mark.parametrize("case,mode", FUSED_PAIRS, ids=[f"{c.name}-{m}" for c, m in FUSED_PAIRS])
def test_long_run_equals_eager_steps(eng, case, mode, n, ragged):
    chain(eng, case, mode, n, ragged)


@pytest.mark.parametrize("ragged", [False, True], ids=["whole", "ragged"])
@pytest.mark.parametrize("n", rc.CHAIN_COUNTS_UNFUSED)
@pytest.mark.parametrize("case", UNFUSED_CASES, ids=[c.name for c in UNFUSED_CASES])
def test_long_unfused_sgld_run_equals_eager_steps(eng, case, n, ragged):
    chain(eng, case, "sgld", n, ragged)


@pytest.mark.parametrize("mode", ["sgd", "swag", "bbb"])
@pytest.mark.parametrize("case", UNFUSED_CASES, ids=[c.name for c in UNFUSED_CASES])
def test_unfused_model_is_refused_by_the_other_runs(eng, case, mode):
    from bayesian_inference_for_nn_amd._lib import PyzError
    data = data_of(case)
    k, freq = (3, 2) if mode == "swag" else (0, 0)
    call = RunCall(3, 2, case.sizes, tuple(0.5 for _ in case.sizes), k, freq)
    d = Dev(eng, case, mode, data)
    start = rc.initial_state(mode, data, k)
    d.reset(start)
    before = (d.state(), d.outputs())
    with pytest.raises(PyzError) as e:
        d.run(call)
    assert e.value.code == E_INVALID
    assert_same((d.state(), d.outputs()), before, f"{case.name} {mode}: a refused call")
    assert d.guards() == []
    d.close()


# ---------------------------------------------------------------- launches
def probed(eng, d, call):
    with eng.KernelProbe(1024) as kp:
        d.run(call, use_graph=True, side=False)
    assert d.plan.last_run_path() == ("eager", len(call.sizes))      # a probed run launches eagerly
    return [rc._norm(n) for n, _ in kp.launches]


@pytest.mark.parametrize("case,mode", PAIRS, ids=PAIR_IDS)
def test_launches_of_a_run(eng, case, mode):
    data = data_of(case)
    val = mode == "bbb" and case.name != "r_s2"                       # (one BBB case without the validation forward)
    d = Dev(eng, case, mode, data, val=val)
    counts = (3, 33) if case.name in ("r_s4", "r_l1", "r_unfused_d218") else (3,)
    for n in counts:
        first, _ = chain_calls(case, mode, n, ragged=True, val=val)
        d.reset(rc.initial_state(mode, data, first.k))
        got = probed(eng, d, first)
        want = rc.expected_run_launches(case, mode, n, n_val=rc.N_VAL if val else 0)
        assert got == want, (case.name, mode, n, got[:12], want[:12])
        assert got.count("k_bbb_sample") == (mode == "bbb")
    d.close()


# ---------------------------------------------------------------- SWAG and BBB bookkeeping
@pytest.mark.parametrize("book", BOOKS, ids=[b.name for b in BOOKS])
def test_bookkeeping(eng, book):
    case, calls = rc.book_call(book)
    data, mode, call = data_of(case), book.mode, calls[-1]
    d = Dev(eng, case, mode, data, val=book.val)
    start = rc.initial_state(mode, data, book.k)
    if book.before:                       # an earlier call leaves the state this one continues
        d.reset(start)
        d.run(calls[0])
        start = d.state()
        hits = [n for n in range(calls[0].n0, calls[0].n0 + book.before) if n % book.freq == 0]
        assert hits and calls[0].n0 == 0
    end = per_step(d, case, data, call, mode, start, f"{book.name}")
    if mode == "swag":
        first = rc.initial_state(mode, data, book.k)["dev"]
        ns = range(calls[0].n0, call.n0 + book.n_steps)
        hit_rows = {rc.swag_row(n, book.k, book.freq) for n in ns if n % book.freq == 0}
        for r in range(book.k):
            assert (r in hit_rows) != same_bits(end["dev"][r], first[r]), f"{book.name}: deviation row {r} (rows hit: {sorted(hit_rows)})"
        if not hit_rows:
            assert same_bits(end["mean"], start["mean"]) and same_bits(end["sq"], start["sq"])
    d.close()


# ---------------------------------------------------------------- the graph cache and the per-run tables
CACHE_CASE = "r_s4"


def whole(case, mode, n, n0=None, slot0=None, lr_scale=1.0, val=False, k=None, freq=None):
    lr = lr_scale * (case.bbb_lr if mode == "bbb" else case.lr) / 64
    ks, fs = case.swag if mode == "swag" else (0, 0)
    return RunCall(case.n0 if n0 is None else n0, case.slot0 if slot0 is None else slot0, (case.bmax,) * n,
                   tuple(lr * (1.0 - (i % 8) / 16.0) for i in range(n)), ks if k is None else k, fs if freq is None else freq, val)


def graph_equals_eager(d, call, start, what, launches=None):
    """The call from graphs on a side stream against the same steps as eager steps, from `start`: bit for bit."""
    d.reset(start)
    d.eager(call)
    want = (d.state(), d.outputs())
    d.reset(start)
    d.run(call)
    assert d.plan.last_run_path() == ("graph", len(call.sizes)), what
    assert d.plan.last_run_graph_launches() == (launches or len(rc.graph_chunks(len(call.sizes)))), what
    assert_same((d.state(), d.outputs()), want, what)
    assert d.guards() == [], what
    return want


@pytest.mark.parametrize("mode", ["sgld", "swag", "bbb"])
def test_graph_cache(eng, mode):
    case = rc.CASE_BY_NAME[CACHE_CASE]
    data = data_of(case)
    val = mode == "bbb"
    d = Dev(eng, case, mode, data, slots=60, val=val)
    start = rc.initial_state(mode, data, case.swag[0])
    W = lambda n, **kw: whole(case, mode, n, val=val, **kw)
    # 1. the same call twice
    for rep in range(2):
        graph_equals_eager(d, W(5), start, f"{mode}: the same call, time {rep}")
    # 2. nine remainder lengths in turn (seven slots: two have been evicted), then the first again
    lengths = [5, 1, 2, 3, 4, 6, 7, 8, 9]
    assert len(lengths) > rc.GRAPH_CHUNKS - 1
    for n in lengths + [5]:
        graph_equals_eager(d, W(n), start, f"{mode}: remainder length {n}")
    # 3. another theta buffer, another loss buffer, another row table: results in the new ones, the old ones untouched
    key = "mu" if mode == "bbb" else "theta"
    for what in ("theta", "losses", "row table"):
        d.reset(start)
        d.run(W(5))
        old = {"theta": d.bufs[key], "losses": d.out, "row table": d.tab}[what]
        kept = old.get()
        if what == "theta":
            d.bufs[key] = Guarded(start[key], case.aligned)
        elif what == "losses":
            d.out = Block(np.full(tuple(d.out.t.shape), FILL, np.float32))
        else:
            d.tab = Block(data.tab[60:120], torch.int32, sentinel=1)
        assert {"theta": d.bufs[key], "losses": d.out, "row table": d.tab}[what].t.data_ptr() != old.t.data_ptr()
        for n in (5, 33):
            graph_equals_eager(d, W(n), start, f"{mode}: another {what} buffer, {n} steps")
        torch.cuda.synchronize()
        assert np.array_equal(old.get().view(np.int32), kept.view(np.int32)), f"{mode}: the old {what} buffer was written"
        assert old.intact()
    # 4. another seed
    d.seed = case.seed + 1
    other = graph_equals_eager(d, W(5), start, f"{mode}: another seed")
    d.seed = case.seed
    mine = graph_equals_eager(d, W(5), start, f"{mode}: the first seed again")
    assert (mode == "swag") == same_bits(other[0][key], mine[0][key])
    # 5. another alpha and prior (BBB), another k and frequency (SWAG)
    if mode == "bbb":
        d.alpha, d.prior = 0.125, (0.25, 0.5)
        other = graph_equals_eager(d, W(5), start, "bbb: another alpha and prior")
        assert not same_bits(other[0]["mu"], mine[0]["mu"])
        d.alpha, d.prior = case.step.alpha, case.step.prior
    if mode == "swag":
        k2 = rc.initial_state(mode, data, 2)
        graph_equals_eager(d, W(5, k=2, freq=1), k2, "swag: another k")
        graph_equals_eager(d, W(5, k=2, freq=2), k2, "swag: another frequency")
        graph_equals_eager(d, W(5), start, "swag: the first k and frequency again")
    # 6. the same key with other learning rates, batch sizes (the same largest one), count and slots
    graph_equals_eager(d, W(5), start, f"{mode}: before the table changes")
    graph_equals_eager(d, W(5, lr_scale=0.5), start, f"{mode}: other learning rates")
    graph_equals_eager(d, W(5, n0=case.n0 + 7), start, f"{mode}: another count")
    graph_equals_eager(d, W(5, slot0=case.slot0 + 9), start, f"{mode}: another slot0")
    ragged = W(5)._replace(sizes=(case.bmax, 23, case.bmax, 1, 7))
    d.reset(start)
    d.run(ragged, use_graph=False)
    want = (d.state(), d.outputs())
    d.reset(start)
    d.run(ragged)
    assert d.plan.last_run_path() == ("graph", 5)
    assert_same((d.state(), d.outputs()), want, f"{mode}: other batch sizes under the same graph")
    d.reset(start)
    d.eager(ragged)
    assert_same(want, (d.state(), d.outputs()), f"{mode}: other batch sizes against eager steps", exact=False)
    # 8. a run on the default stream is eager-chained
    d.reset(start)
    d.eager(W(5))
    want = (d.state(), d.outputs())
    d.reset(start)
    d.run(W(5), use_graph=True, side=False)
    assert d.plan.last_run_path() == ("eager", 5) and d.plan.last_run_graph_launches() == 0
    assert_same((d.state(), d.outputs()), want, f"{mode}: default stream")
    d.plan.check_finite()
    d.close()


@pytest.mark.parametrize("mode", ["sgld", "swag", "bbb"])
def test_four_pinned_table_runs_back_to_back(eng, mode):
    """7. Four runs of 33 steps (tables through the two pinned staging buffers, used in turn) with different learning-rate
    tables, enqueued on one stream with no host synchronisation in between, against 132 eager steps."""
    case = rc.CASE_BY_NAME[CACHE_CASE]
    data = data_of(case)
    val = mode == "bbb"
    d = Dev(eng, case, mode, data, slots=140, val=val)
    start = rc.initial_state(mode, data, case.swag[0])
    calls = [whole(case, mode, 33, val=val, lr_scale=1.0)]
    for scale in (0.5, 0.75, 0.25):
        nxt = whole(case, mode, 33, val=val, lr_scale=scale)
        calls.append(after(calls[-1], nxt.sizes, nxt.lrs))
    assert len({c.lrs for c in calls}) == 4 and all(rc.table_transport(len(c.sizes)) == "pinned" for c in calls)
    d.reset(start)
    for c in calls:
        d.eager(c)
    want = (d.state(), d.outputs())
    d.reset(start)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    for c in calls:
        d.run_on(st, c)
    st.synchronize()
    assert_same((d.state(), d.outputs()), want, f"{mode}: four runs of 33 steps back to back")
    assert written_slots(case, mode, want[1][0]) == list(range(case.slot0, case.slot0 + 132))
    assert d.guards() == []
    d.plan.check_finite()
    d.close()


# ---------------------------------------------------------------- the run-wide switches (read once: a child process)
SWITCH_CASES = [("r_s2", "sgd"), ("r_s4_xcd12", "swag"), ("r_s8_xcd8_l3_mse", "sgld"), ("r_s4", "bbb"), ("r_unfused_d1100", "sgld")]
SWITCHES = [("PYZ_BBB_FUSE_SAMPLE", "0"), ("PYZ_BATCH_AHEAD", "0"), ("PYZ_BATCH_AHEAD", "2")]
_switch = {}


def switch_results(eng):
    """One case per mode (and the unfused SGLD run): 33 steps, whole batches; computed once per process."""
    if not _switch:
        for name, mode in SWITCH_CASES:
            case = rc.CASE_BY_NAME[name]
            data = data_of(case)
            val = mode == "bbb"
            d = Dev(eng, case, mode, data, val=val)
            d.reset(rc.initial_state(mode, data, case.swag[0]))
            d.run(whole(case, mode, 33, val=val))
            assert d.plan.last_run_path() == ("graph", 33)
            state, (out, vals) = d.state(), d.outputs()
            for key, v in state.items():
                _switch[f"{name}.{mode}.{key}"] = v
            _switch[f"{name}.{mode}.losses"], _switch[f"{name}.{mode}.vals"] = out, vals
            d.close()
    return _switch


def child_main(path):
    from bayesian_inference_for_nn_amd import engine
    np.savez(path, **switch_results(engine))


@pytest.mark.parametrize("switch,value", SWITCHES, ids=[f"{k}={v}" for k, v in SWITCHES])
def test_a_run_wide_switch_gives_the_same_bits(eng, tmp_path, switch, value):
    """PYZ_BBB_FUSE_SAMPLE=0: k_bbb_sample in every step of the graph instead of the sample in the epilogue before.
    PYZ_BATCH_AHEAD=0: every step gathers its own rows; =2: ahead whatever the tile count.  Read once: a child process."""
    assert not os.environ.get(switch)
    path = str(tmp_path / "switched.npz")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_run_matrix as t; t.child_main({path!r})")
    flags = ["-s"] if sys.flags.no_user_site else []
    res = subprocess.run([sys.executable, *flags, "-c", code], env=dict(os.environ, **{switch: value}),
                         capture_output=True, text=True, timeout=180)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    theirs, ours = np.load(path), switch_results(eng)
    assert sorted(theirs.files) == sorted(ours)
    for key in ours:
        assert same_bits(theirs[key], ours[key]), key


def test_the_switch_runs_are_the_eager_steps(eng):
    ours = switch_results(eng)
    for name, mode in SWITCH_CASES:
        case = rc.CASE_BY_NAME[name]
        data = data_of(case)
        val = mode == "bbb"
        d = Dev(eng, case, mode, data, val=val)
        d.reset(rc.initial_state(mode, data, case.swag[0]))
        d.eager(whole(case, mode, 33, val=val))
        state, (out, vals) = d.state(), d.outputs()
        for key, v in state.items():
            assert same_bits(ours[f"{name}.{mode}.{key}"], v), (name, mode, key)
        assert same_bits(ours[f"{name}.{mode}.losses"], out) and same_bits(ours[f"{name}.{mode}.vals"], vals)
        d.close()


# ---------------------------------------------------------------- the non-finite sentinel
FINITE = [("r_s2", "sgd"), ("r_s2", "swag"), ("r_s2", "sgld"), ("r_s2", "bbb"), ("r_unfused_d1100", "sgld")]


@pytest.mark.parametrize("name,mode", FINITE, ids=[f"{n}-{m}" for n, m in FINITE])
def test_check_finite_sees_a_diverged_run(eng, name, mode):
    """include/pyz.h: every kernel that finalises a step's loss counts NaN / Inf results for pyz_check_finite -- in a chained
    run as well.  An infinite learning rate throws every parameter out of float32's range in the first step: its own loss is
    still finite, every later one is not."""
    from bayesian_inference_for_nn_amd._lib import E_NAN, PyzError
    case = rc.CASE_BY_NAME[name]
    data = data_of(case)
    d = Dev(eng, case, mode, data)
    start = rc.initial_state(mode, data, case.swag[0])
    d.reset(start)
    d.run(whole(case, mode, 6))
    out, _ = d.outputs()
    assert np.all(np.isfinite(out[case.slot0:case.slot0 + 6]))
    d.plan.check_finite()
    d.reset(start)
    wild = whole(case, mode, 6)._replace(lrs=(float("inf"),) * 6)
    d.run(wild)
    out, _ = d.outputs()
    got = out[case.slot0:case.slot0 + 6, 0] if mode == "bbb" else out[case.slot0:case.slot0 + 6]
    assert np.isfinite(got[0]) and not np.any(np.isfinite(got[1:])), got
    with pytest.raises(PyzError) as e:
        d.plan.check_finite()
    assert e.value.code == E_NAN
    d.plan.check_finite()      # the count was reset
    assert d.guards() == []
    d.close()
