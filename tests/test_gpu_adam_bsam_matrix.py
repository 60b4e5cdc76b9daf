"""Every eager ADAM, VADAM and BSAM step path against the float64 restatement (tests/adam_bsam_cases.py lists the cases and
cells), and the device-resident runs of the fused cases against those eager steps.

A test is one (case, kind): three consecutive steps on one plan, per noise variant of the kind.  Before every step the state
is read back and the reference restarts from it, so nothing accumulates and every bound is a bound on one step.  Per step:
the launches (k_wgrad_adam<S> / k_wgrad_bsam<S, 0 | 1> of the table on the fused path; k_dense_bwd_weight_sq per layer with
k_adam_update, or k_dense_bwd_weight per layer and pass with k_bsam_ascent and k_bsam_update, on the other; the perturbation
kernels), so a change in dispatch fails the case instead of quietly testing another kernel; then
adam_bsam_cases.compare_step (update, m, v per layer block, BSAM's ascent point, v = s element by element on the one-layer
cases, the losses); the sentinels around every state buffer; that repeating the step from the same state gives the same
bits; and, where the device draws the noise, that the step with the same Philox stream injected gives the same bits.  The
whole (case, kind) then runs again on a plan whose rows past the batch, and on an x whose rows outside the batch, hold NaN:
not a bit may change.  (KernelProbe reports kernel expressions, not block sizes: the S of k_dense_bwd_weight_sq, and with
it the wave of 21 steps, is the restated one, pinned to the source by tests/test_adam_bsam_dispatch_table.py.)"""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import adam_bsam_cases as ab  # noqa: E402
from adam_bsam_cases import CASES, KINDS, N_STEPS, STREAM, VARIANTS, compare_step, expected_ab_launches, ref_step  # noqa: E402
from dense_cases import ENV_FORBIDDEN  # noqa: E402
from oracle import philox as o_philox  # noqa: E402

SENTINEL = -12345.0
TAIL = 64
EXTRA_ROWS = 3   # rows appended to x in the poisoned run
WORST = {}       # kind -> (largest error / tolerance, case, variant, quantity): printed at the end of the module
SEEN = set()     # kernel expressions the probes of this module reported
RAN = set()
WATCHED = ("k_wgrad_adam", "k_wgrad_bsam", "k_dense_bwd_weight", "k_adam_update", "k_bsam_ascent", "k_bsam_update",
           "k_vadam_perturb", "k_bsam_perturb", "k_wgrad_all")


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = [k for k in ENV_FORBIDDEN if os.environ.get(k)]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the library reads them once per process and every "
                    "expected launch of this module assumes their defaults -- unset them")
    from bayesian_inference_for_nn_amd import engine
    yield engine
    for kind, (ratio, name, variant, q) in sorted(WORST.items()):
        print(f"WORST | {kind} | error / tolerance {ratio:.4f} | {name} | {variant} | {q}")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Guarded:
    """A (D) float32 vector as a view into a sentinel-filled buffer: one element in front (the view then sits 4 bytes off
    16-byte alignment) or four (aligned), 64 behind."""

    def __init__(self, values, aligned):
        values = np.asarray(values, dtype=np.float32).reshape(-1)
        self.lead, self.D = (4 if aligned else 1), values.size
        self.buf = torch.full((self.lead + self.D + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.lead:self.lead + self.D]
        self.t.copy_(dev(values))
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (0 if aligned else 4) and self.t.is_contiguous()

    def set(self, values):
        self.t.copy_(dev(values))

    def get(self):
        return self.t.cpu().numpy().copy()

    def intact(self):
        return bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[self.lead + self.D:] == SENTINEL).all())


def launched(kp):
    names = tuple(n.replace(" ", "") for n, _ in kp.launches)
    SEEN.update(names)
    return tuple(n for n in names if n.startswith(WATCHED))


def squeezed(names):
    return tuple(n.replace(" ", "") for n in names)


class Run:
    """The device side of one (case, kind): plan, data and guarded state buffers; `step` runs step k of a variant.
    poison: the plan's rows past the batch and the rows of x outside the batch hold NaN."""

    def __init__(self, eng, case, kind, poison=False):
        self.eng, self.case, self.kind, self.data = eng, case, kind, ab.ab_data(case)
        data, spec = self.data, case.spec
        self.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.max_batch)
        x, y = data.x, data.y
        ydt = torch.int32 if spec.loss == "scce" else torch.float32
        if poison:
            inside = np.zeros(len(x) + EXTRA_ROWS, dtype=bool)
            inside[data.idx if data.idx is not None else np.arange(case.batch)] = True
            x = np.concatenate([x, np.zeros((EXTRA_ROWS, x.shape[1]), dtype=np.float32)])
            x[~inside] = np.nan
            y = np.concatenate([y, np.zeros((EXTRA_ROWS,) + y.shape[1:], dtype=y.dtype)])
            if spec.loss != "scce":
                y[~inside] = np.nan
            # every row of the plan's activations, deltas and batch copy: one gradient call over max_batch rows of NaN
            nan_x = torch.full((case.max_batch, spec.dims[0]), float("nan"), device="cuda")
            nan_th = torch.full((case.D,), float("nan"), device="cuda")
            self.plan.loss_grad(nan_th, nan_x, dev(y[:1].repeat(case.max_batch, axis=0), ydt), batch=case.max_batch)
            torch.cuda.synchronize()
            try:
                self.plan.check_finite()     # (that call's loss is NaN: read the count, which resets it)
            except Exception:
                pass
        self.x, self.y = dev(x), dev(y, ydt)
        self.rid = dev(data.idx, torch.int32) if data.idx is not None else None
        self.bufs = {q: Guarded(v, case.aligned) for q, v in ab.initial_state(kind, data).items()}
        self.noise = Guarded(np.zeros(case.D), case.aligned)
        self.out = torch.zeros(2, device="cuda")
        self.launches = None

    def set_state(self, s):
        for q, v in s.items():
            self.bufs[q].set(v)

    def get_state(self):
        return {q: b.get() for q, b in self.bufs.items()}

    def guards_intact(self):
        return [q for q, b in list(self.bufs.items()) + [("eps", self.noise)] if not b.intact()]

    def step(self, k, noise, probe=False):
        """Step k with `noise` injected (a float32 vector, a device tensor, or None: the device draws it, or the kind has
        none); returns the state after it with "loss" (and VADAM's "pert").  probe: self.launches = (perturb, sequence)."""
        c, b, kind = self.case, self.bufs, self.kind
        kw = dict(batch=c.batch, row_idx=self.rid)
        z = None
        if noise is not None:
            self.noise.t.copy_(noise if isinstance(noise, torch.Tensor) else dev(noise))
            z = self.noise.t
        self.out.zero_()
        got, first, second = {}, (), ()
        step = ab.philox_step(c, k)
        if kind == "bsam":
            h = ab.bsam_hyper(c, k)
            call = lambda: self.plan.bsam_step(b["theta"].t, b["m"].t, b["v"].t, self.x, self.y, step=step, seed=c.seed,
                                               loss_out=self.out, eps=z, **h, **kw)
            if probe:
                with self.eng.KernelProbe(64) as kp:
                    call()
                names = launched(kp)
                first, second = names[:1], names[1:]
            else:
                call()
        else:
            h = ab.adam_hyper(c, kind, k)
            if kind == "vadam":
                pert = lambda: self.plan.vadam_perturb(b["theta"].t, b["v"].t, h["lam"], h["num_data"], step, c.seed, eps=z)
                if probe:
                    with self.eng.KernelProbe(8) as kp:
                        pert()
                    first = squeezed(n for n, _ in kp.launches)     # the call launches nothing else
                    SEEN.update(first)
                else:
                    pert()
                got["pert"] = b["theta"].get()
            call = lambda: self.plan.adam_step(b["theta"].t, b["m"].t, b["v"].t, self.x, self.y, h["lr"], h["beta_1"], h["beta_2"],
                                               h["epoch"], self.out[:1], denom_eps=h["denom_eps"], decay=h["decay"], **kw)
            if probe:
                with self.eng.KernelProbe(64) as kp:
                    call()
                second = launched(kp)
            else:
                call()
        self.launches = (first, second)
        got.update(self.get_state())
        o = self.out.cpu().numpy().copy()
        got["loss"] = o[:2] if kind == "bsam" else o[:1]
        return got


def same_bits(a, b):
    return a.keys() == b.keys() and all(
        np.array_equal(np.asarray(a[q], dtype=np.float32).view(np.int32), np.asarray(b[q], dtype=np.float32).view(np.int32)) for q in a)


def run_case(eng, case, kind, poison, check):
    """The three chained steps of every variant; returns [(variant, k, got)].  check: everything but the bits is judged."""
    run = Run(eng, case, kind, poison)
    exp = expected_ab_launches(case, kind)
    data = run.data
    worst, out = {}, []
    for variant in VARIANTS[kind]:
        run.set_state(ab.initial_state(kind, data))
        for k in range(N_STEPS):
            what = f"{case.name} {kind} {variant} step {k}"
            s0 = run.get_state()
            inj = ab.injected_noise(case, kind, variant, k)
            got = run.step(k, inj, probe=check)
            out.append((variant, k, got))
            if not check:
                continue
            # 1. the launches
            assert run.launches == (squeezed(exp.perturb), squeezed(exp.sequence)), (what, run.launches, exp)
            # 2. update, m, v, the ascent point and the losses against the float64 reference restarted from s0
            ref = ref_step(case, kind, s0, k, variant=variant, pert=got.get("pert"))
            rep = compare_step(case, kind, k, s0, got, ref, what=f"{variant}: ")
            for q, r in sorted(rep.items()):
                print(f"{what}: {q}: error / tolerance {r:.4f}")
                worst[q] = max(worst.get(q, 0.0), r)
                if r > WORST.get(kind, (-1.0,))[0]:
                    WORST[kind] = (r, case.name, variant, q)
            # 3. the sentinels around every buffer
            assert run.guards_intact() == [], f"{what}: wrote outside {run.guards_intact()}"
            # 4. the same step from the same state: the same bits
            run.set_state(s0)
            again = run.step(k, inj)
            assert same_bits(got, again), f"{what}: repeating the step from the same state gives other bits"
            # 5. the device's own draws are the Philox stream fill_normal writes, element by element, and that stream is
            # the oracle's to the bound the comparison's reference relies on
            if variant == "device":
                z = eng.fill_normal(torch.empty(case.D, device="cuda"), case.seed, STREAM[kind], ab.philox_step(case, k))
                run.set_state(s0)
                injected = run.step(k, z)
                assert same_bits(got, injected), f"{what}: device noise and the injected stream give different bits"
                zo = o_philox.normal(case.seed, STREAM[kind], ab.philox_step(case, k), case.D)
                assert np.abs(z.cpu().numpy().astype(np.float64) - zo).max() <= ab.BOX_MULLER_ABS, what
            assert run.guards_intact() == [], f"{what}: wrote outside {run.guards_intact()}"
    if check:
        run.plan.check_finite()
        print(f"CASE | {case.name} | {kind} | " + " | ".join(f"{q} {r:.4f}" for q, r in sorted(worst.items())))
    run.plan.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_ab_case(eng, case, kind):
    clean = run_case(eng, case, kind, poison=False, check=True)
    RAN.add((case.name, kind))
    # rows of the plan past the batch and rows of x outside the batch: NaN there does not change a bit
    dirty = run_case(eng, case, kind, poison=True, check=False)
    assert [(v, k) for v, k, _ in clean] == [(v, k) for v, k, _ in dirty]
    for (variant, k, a), (_, _, b) in zip(clean, dirty):
        assert same_bits(a, b), f"{case.name} {kind} {variant} step {k}: NaN in rows outside the batch changes the result"


def test_every_kernel_of_the_table_was_launched(eng):
    """With every (case, kind) of this module run in this process: the probes reported each kernel the issue names."""
    if len(RAN) < len(CASES) * len(KINDS):
        return      # a selection of cases was run: nothing to conclude
    want = {f"k_wgrad_adam<{S}>" for S in ab.SS} | {f"k_wgrad_bsam<{S},{p}>" for S in ab.SS for p in (0, 1)}
    want |= {"k_dense_bwd_weight_sq", "k_dense_bwd_weight", "k_adam_update", "k_bsam_ascent", "k_bsam_update",
             "k_vadam_perturb", "k_bsam_perturb"}
    assert want <= SEEN, sorted(want - SEEN)
    assert not any(n.startswith("k_wgrad_all") for n in SEEN), "an ADAM / VADAM / BSAM step ran k_wgrad_all"


# ---------------------------------------------------------------- the device-resident runs of the fused cases
FUSED = [c for c in CASES if c.fused]


def run_hyper(case, kind):
    """A run has one set of betas; lr and the epoch change per step: the third step's hyper-parameters (decay, another
    denom_eps; BSAM: both betas 0.5) with the three steps' learning rates and epochs."""
    if kind == "bsam":
        return ab.bsam_hyper(case, 2), [ab.bsam_hyper(case, k)["lr"] for k in range(N_STEPS)], None
    h = ab.adam_hyper(case, kind, 2)
    return h, [ab.adam_hyper(case, kind, k)["lr"] for k in range(N_STEPS)], [ab.adam_hyper(case, kind, k)["epoch"] for k in range(N_STEPS)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", FUSED, ids=[c.name for c in FUSED])
def test_run_equals_eager_steps(eng, case, kind):
    """Three steps through adam_run / bsam_run, graph and no graph, against the three eager steps on the same row table:
    bit for bit (the entry points as tests/test_gpu_adam_bsam_run.py calls them; device noise)."""
    data, spec = ab.ab_data(case), case.spec
    plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.max_batch)
    x, y = dev(data.x), dev(data.y, torch.int32 if spec.loss == "scce" else torch.float32)
    rows = data.idx if data.idx is not None else np.arange(case.batch, dtype=np.int32)
    tab = np.zeros((N_STEPS, case.max_batch), dtype=np.int32)
    tab[:, :case.batch] = rows
    tab_d, row_d = dev(tab, torch.int32), dev(rows, torch.int32)
    h, lrs, epochs = run_hyper(case, kind)
    per = 2 if kind == "bsam" else 1
    step0 = ab.philox_step(case, 0)
    s0 = ab.initial_state(kind, data)

    def fresh():
        return [dev(s0[q]) for q in ("theta", "m", "v")], torch.zeros(per * N_STEPS, device="cuda")

    (th, m, v), losses = fresh()
    for i in range(N_STEPS):
        kw = dict(batch=case.batch, row_idx=row_d)
        if kind == "bsam":
            plan.bsam_step(th, m, v, x, y, **dict(h, lr=lrs[i]), step=step0 + i, seed=case.seed, loss_out=losses[2 * i:2 * i + 2], **kw)
            continue
        if kind == "vadam":
            plan.vadam_perturb(th, v, h["lam"], h["num_data"], step0 + i, case.seed)
        plan.adam_step(th, m, v, x, y, lrs[i], h["beta_1"], h["beta_2"], epochs[i], losses[i:i + 1], denom_eps=h["denom_eps"],
                       decay=h["decay"], **kw)
    want = [t.cpu().numpy() for t in (th, m, v, losses)]
    plan.check_finite()
    assert np.all(np.isfinite(want[3])) and not np.array_equal(want[0], s0["theta"])
    for use_graph in (True, False):
        (th, m, v), losses = fresh()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            if kind == "bsam":
                plan.bsam_run(th, m, v, x, y, tab_d, [case.batch] * N_STEPS, lrs, h["beta_1"], h["beta_2"], h["lam"], h["rho"],
                              h["gam"], h["num_data"], step0, case.seed, losses, use_graph=use_graph)
            else:
                vd = kind == "vadam"
                plan.adam_run(th, m, v, x, y, tab_d, [case.batch] * N_STEPS, lrs, epochs, h["beta_1"], h["beta_2"], losses,
                              denom_eps=h["denom_eps"], decay=h["decay"], perturb=vd, lam=h["lam"] if vd else 0.0,
                              num_data=h["num_data"] if vd else 1.0, step0=step0, seed=case.seed, use_graph=use_graph)
        stream.synchronize()
        plan.check_finite()
        assert plan.last_run_path() == ("graph" if use_graph else "eager", N_STEPS)
        got = [t.cpu().numpy() for t in (th, m, v, losses)]
        for g, w, nm in zip(got, want, ("theta", "m", "v", "losses")):
            assert np.array_equal(g.view(np.int32), w.view(np.int32)), \
                f"{case.name} {kind} graph={use_graph}: {nm} differs from the eager steps (max {np.abs(g - w).max():.3e})"
    plan.close()
