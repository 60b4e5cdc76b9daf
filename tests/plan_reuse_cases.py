"""The op table of tests/test_gpu_plan_reuse.py: every entry point of engine.MLPPlan as a named op that can be called again
and again on ONE plan (a plain module: importing it needs neither torch nor a device; `build_ops` does).

What is under test is the plan as a stateful object (csrc/pyz_api.hip): its four graph caches, the buffers ensure_bytes
frees and reallocates when a call asks for more particles, the pending lazy StepCtl, grad_owner / km_valid, the batch
assembled one step ahead, the non-finite sentinel, act[] / delta[].  An op owns its seeded device tensors, restores them
IN PLACE (`reset`: the addresses persist, so a second call meets the same graph key) and returns every output and every
state tensor as host arrays (`call`).  The reference of an op is the same op on a fresh plan; the arithmetic itself is
pinned to the float64 oracle by the per-kernel test files.

Shapes: the smallest that reach both step paths -- `narrow` (last layer <= 32 units: can_fuse) and `wide` (33 units: the
unfused sequence that bakes the plan's gradient buffer into the chained SGLD graphs) -- and a one-unit MSE model for
fsvi_step.  Every plan: max_batch 8, max_particles 4; 11 data rows; runs of 5 steps with batches 8, 8, 3, 8, 8 (SGLD-family
runs: one remainder graph of five steps; ADAM / BSAM runs: three graphs, cut where the batch size changes)."""

from __future__ import annotations

import zlib
from typing import Callable, NamedTuple

import numpy as np

MAX_BATCH, MAX_PARTICLES, N_ROWS = 8, 4, 11
SIZES = (8, 8, 3, 8, 8)
LRS = (0.05, 0.04, 0.03, 0.02, 0.01)
N_STEPS = len(SIZES)
SLOTS = N_STEPS + 1
P = 3                      # chains / lanes / particles of the particle-batched ops
DRAWS = 5                  # rows of the read-outs' weights: one chunk of max_particles and a rest of one
SENTINEL = -12345.0
SLICED_ROWS = 192          # pyz_hmc_step: two slices of 96 rows (PYZ_HMC_ROWS_PER_WG), the smallest data set of the sliced forms
ADAM_RUN_GRAPHS = 3        # adam_run_impl: a graph holds steps of one batch size -> [8, 8], [3], [8, 8] (other StepCtl slot)


def first_call_info(name: str) -> dict:
    """What the info calls report of an op's first call on a fresh plan (every later call of it alone: captures 0).
    sgld_run_impl: one remainder graph of N_STEPS steps; adam_run_impl: ADAM_RUN_GRAPHS graphs; pyz_hmc_run at 8 rows: the
    one-workgroup form, every proposal eager."""
    if name in ("adam_run", "bsam_run"):
        return dict(path=("graph", N_STEPS), launches=ADAM_RUN_GRAPHS, captures=ADAM_RUN_GRAPHS)
    if name in ("hmc_run_p1", "sgld_run_eager"):
        return dict(path=("eager", N_STEPS), launches=0, captures=0)
    return dict(path=("graph", N_STEPS), launches=1, captures=1)


class Spec(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str

    @property
    def D(self) -> int:
        return sum((i + 1) * o for i, o in zip(self.dims[:-1], self.dims[1:]))

    @property
    def can_fuse(self) -> bool:
        return self.dims[-1] <= 32


SPECS = {s.name: s for s in (Spec("narrow", (6, 9, 4), ("tanh", "softmax"), "scce"),
                             Spec("wide", (6, 9, 33), ("tanh", "softmax"), "scce"),
                             Spec("mse1", (6, 9, 1), ("tanh", "linear"), "mse"))}

# ---------------------------------------------------------------- the table
FORWARD = ("forward", "loss_grad")
EAGER_STEPS = ("sgd_step", "swag_step", "sgld_step", "adam_step", "bsam_step", "bbb_step")
SGLD_RUNS = ("sgld_run_graph", "sgld_run_eager")
CHAINED_RUNS = ("sgd_run", "swag_run", "bbb_run", "adam_run", "bsam_run")      # refused without can_fuse
ROWS = ("sgld_chains_step", "sgld_chains_run", "sgld_lanes_run", "lane_scores")
HMC = ("hmc_step_p1", "hmc_step_p3", "hmc_run_p1")
SVGD = ("svgd_step", "svgd_grad_sweep")
READOUTS = ("predict", "predict_moments", "predict_surface", "input_grad")
ALL_OPS = FORWARD + EAGER_STEPS + SGLD_RUNS + CHAINED_RUNS + ROWS + HMC + SVGD + READOUTS

# sgld_run_impl / adam_run_impl: "the chained ... runs need a last layer of at most 32 units"
REFUSED = {"narrow": (), "wide": CHAINED_RUNS}
TABLE = {name: tuple(o for o in ALL_OPS if o not in REFUSED[name]) for name in ("narrow", "wide")}
# the one-unit MSE model: fsvi_step among one op of every family (the full table runs on the two softmax models)
TABLE["mse1"] = ("fsvi_step", "loss_grad", "sgd_step", "bbb_step", "sgld_run_graph", "adam_run", "sgld_chains_step",
                 "lane_scores", "hmc_step_p3", "svgd_step", "predict", "input_grad")

# ops that replay captured graphs on a stream of the caller's own (m->graphs; adam_graphs; hmc_run_graphs)
GRAPH_OPS = ("sgld_run_graph", "sgd_run", "swag_run", "bbb_run", "adam_run", "bsam_run", "hmc_run_p1")
# the cache an op's graphs live in, and the info call that counts its captures.  A cache holds the graphs of ONE key (the
# caller's pointers and scalars): another op of the same cache replaces them, and the first op captures again.
GRAPH_CACHE = {"sgld_run_graph": "graphs", "sgld_run_eager": "graphs", "sgd_run": "graphs", "swag_run": "graphs", "bbb_run": "graphs",
               "adam_run": "adam_graphs", "bsam_run": "adam_graphs", "hmc_run_p1": "hmc_run_graphs"}
CAPTURES_OF = {"graphs": "sgld_run_captures", "adam_graphs": "adam_run_captures", "hmc_run_graphs": "hmc_run_captures"}
# ops that ask the plan for (P, D) scratch of P = 3 rows (need_grad / need_grad2 / need_qsave with P): behind any graph op
# of the table -- all of them single-chain -- the plan's workspace must grow across them
GROWING_OPS = ("sgld_chains_step", "sgld_chains_run", "sgld_lanes_run", "hmc_step_p3", "svgd_step", "svgd_grad_sweep", "fsvi_step")
# (spec, A, B): B moves a buffer A's run allocated -- ensure_bytes frees it and drops every graph cache of the plan
MOVING_TRIPLES = (("wide", "sgld_run_graph", "svgd_grad_sweep"),     # m->grad, baked into the unfused chained SGLD step
                  ("narrow", "bbb_run", "sgld_chains_step"),         # m->grad = the second weight buffer of the fused sampling
                  ("narrow", "bsam_run", "hmc_step_p3"),             # m->grad2 = the first pass's gradient
                  ("narrow", "hmc_run_p1", "svgd_step"))             # m->grad of the proposals
LAZY_CTL_FOLLOWERS = READOUTS + ("lane_scores",)


def graph_ops(spec_name: str) -> tuple:
    return tuple(o for o in GRAPH_OPS if o in TABLE[spec_name])


# ---------------------------------------------------------------- data
class Data(NamedTuple):
    x: np.ndarray            # (N_ROWS, in)
    y: np.ndarray            # scce: int32 (N_ROWS,); mse: float32 (N_ROWS, 1)
    tab: np.ndarray          # (SLOTS, MAX_BATCH) int32 row table of the runs: every entry a valid row
    idx: np.ndarray          # (MAX_BATCH,) int32 rows of the eager steps' batch


def data(spec: Spec, n_rows: int = N_ROWS, max_batch: int = MAX_BATCH) -> Data:
    rng = np.random.default_rng(zlib.crc32(f"{spec.name}/{n_rows}".encode()))
    x = rng.normal(size=(n_rows, spec.dims[0])).astype(np.float32)
    y = (rng.integers(0, spec.dims[-1], size=n_rows).astype(np.int32) if spec.loss == "scce"
         else rng.normal(size=(n_rows, spec.dims[-1])).astype(np.float32))
    tab = np.stack([rng.permutation(n_rows)[:max_batch] for _ in range(SLOTS)]).astype(np.int32)
    idx = rng.permutation(n_rows)[:MAX_BATCH].astype(np.int32)
    return Data(x, y, tab, idx)


class Env:
    """What the ops of one spec share on the device: the data, two side streams (the legacy default stream cannot be
    captured) and the engine.  n_rows / max_batch: SLICED_ROWS for the plans whose HMC proposals take the sliced form."""

    def __init__(self, spec: Spec, torch, engine, n_rows: int = N_ROWS, max_batch: int = MAX_BATCH):
        self.spec, self.torch, self.engine, self.max_batch = spec, torch, engine, max_batch
        d = data(spec, n_rows, max_batch)
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
        self.x, self.y, self.tab, self.idx = dev(d.x), dev(d.y), dev(d.tab), dev(d.idx)
        self.x8, self.y8 = dev(d.x[:max_batch]), dev(d.y[:max_batch])     # contiguous rows for the entries without a row gather
        self.stream, self.stream2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()

    def plan(self):
        e = self.engine
        return e.MLPPlan(e.MLPSpec(self.spec.dims, self.spec.acts, self.spec.loss), max_batch=self.max_batch, max_particles=MAX_PARTICLES)


class Op:
    """name; `init`: its state and input tensors as host arrays; fn(plan, env, t) -> dict of further output tensors."""

    def __init__(self, name: str, init: dict, fn: Callable):
        self.name, self.init, self.fn = name, init, fn
        self.t = self.t0 = self.env = None

    def alloc(self, env: Env):
        torch = env.torch
        self.env = env
        self.t = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in self.init.items()}
        self.t0 = {k: v.clone() for k, v in self.t.items()}
        torch.cuda.synchronize()
        return self

    def reset(self):
        for k, v in self.t.items():
            v.copy_(self.t0[k])
        self.env.torch.cuda.synchronize()

    def call(self, plan, stream=None) -> dict:
        torch, st = self.env.torch, stream if stream is not None else self.env.stream
        with torch.cuda.stream(st):
            out = self.fn(plan, self.env, self.t) or {}
        st.synchronize()
        res = {k: v.cpu().numpy() for k, v in self.t.items()}
        res.update({f"out.{k}": v.cpu().numpy() for k, v in out.items() if v is not None})
        return res


def same_bits(got: dict, ref: dict) -> list:
    """Names of the arrays of `got` that differ from `ref` in any bit (NaN payloads included)."""
    assert got.keys() == ref.keys()
    return [k for k in ref if got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype or got[k].tobytes() != ref[k].tobytes()]


# ---------------------------------------------------------------- the ops
def _builders(spec: Spec) -> dict:
    D, F = spec.D, spec.dims[0]
    f32 = np.float32

    def rng_of(name):
        return np.random.default_rng(zlib.crc32(f"{spec.name}/{name}".encode()))

    def w(r, *shape):          # weights: small enough for finite softmax rows, large enough for every unit to matter
        return (0.3 * r.normal(size=shape + (D,))).astype(f32)

    def pos(r, *shape):
        return r.uniform(0.01, 0.05, size=shape + (D,)).astype(f32)

    def blank(*shape):
        return np.full(shape, SENTINEL, dtype=f32)

    B = {}

    def op(name):
        def reg(make):
            B[name] = lambda: Op(name, *make(rng_of(name)))
            return make
        return reg

    @op("forward")
    def _(r):
        return dict(theta=w(r, 2)), lambda p, e, t: dict(out=p.forward(t["theta"], e.x, batch=MAX_BATCH, row_idx=e.idx))

    @op("loss_grad")
    def _(r):
        def fn(p, e, t):
            loss, grad = p.loss_grad(t["theta"], e.x, e.y, batch=MAX_BATCH, row_idx=e.idx)
            return dict(loss=loss, grad=grad)
        return dict(theta=w(r, 2)), fn

    @op("sgd_step")
    def _(r):
        return (dict(theta=w(r), loss=blank(1)),
                lambda p, e, t: p.sgd_step(t["theta"], e.x, e.y, 0.05, t["loss"], batch=MAX_BATCH, row_idx=e.idx))

    @op("swag_step")
    def _(r):
        return (dict(theta=w(r), mean=w(r), sq=pos(r), dev_row=w(r), loss=blank(1)),
                lambda p, e, t: p.swag_step(t["theta"], t["mean"], t["sq"], t["dev_row"], e.x, e.y, 0.05, 2, True, t["loss"],
                                            batch=MAX_BATCH, row_idx=e.idx))

    @op("sgld_step")
    def _(r):
        return (dict(theta=w(r), mean=w(r), sq=pos(r), loss=blank(1)),
                lambda p, e, t: p.sgld_step(t["theta"], t["mean"], t["sq"], e.x, e.y, 0.05, 3, 17, t["loss"], batch=MAX_BATCH,
                                            row_idx=e.idx))

    @op("adam_step")
    def _(r):
        return (dict(theta=w(r), m=w(r), v=pos(r), loss=blank(1)),
                lambda p, e, t: p.adam_step(t["theta"], t["m"], t["v"], e.x, e.y, 0.01, 0.9, 0.999, 2, t["loss"], batch=MAX_BATCH,
                                            row_idx=e.idx))

    @op("bsam_step")
    def _(r):
        return (dict(theta=w(r), m=w(r), v=pos(r), loss=blank(2)),
                lambda p, e, t: p.bsam_step(t["theta"], t["m"], t["v"], e.x, e.y, 0.05, 0.9, 0.999, 0.1, 0.05, 0.1, float(N_ROWS), 1,
                                            5, t["loss"], batch=MAX_BATCH, row_idx=e.idx))

    @op("bbb_step")
    def _(r):
        return (dict(mu=w(r), rho=(-3.0 + 0.1 * r.normal(size=D)).astype(f32), w=blank(D), cost=blank(4)),
                lambda p, e, t: p.bbb_step(t["mu"], t["rho"], t["w"], e.x, e.y, 0.01, 0.1, 0.0, 0.5, 2, 9, t["cost"],
                                           batch=MAX_BATCH, row_idx=e.idx))

    def sgld_run(name, use_graph):
        @op(name)
        def _(r):
            return (dict(theta=w(r), mean=w(r), sq=pos(r), losses=blank(SLOTS)),
                    lambda p, e, t: p.sgld_run(t["theta"], t["mean"], t["sq"], e.x, e.y, e.tab, SIZES, LRS, 3, 17, t["losses"],
                                               use_graph=use_graph))
    sgld_run("sgld_run_graph", True)
    sgld_run("sgld_run_eager", False)

    @op("sgd_run")
    def _(r):
        return (dict(theta=w(r), losses=blank(SLOTS)),
                lambda p, e, t: p.sgd_run(t["theta"], e.x, e.y, e.tab, SIZES, LRS, t["losses"]))

    @op("swag_run")
    def _(r):
        return (dict(theta=w(r), mean=w(r), sq=pos(r), dev=w(r, 2), losses=blank(SLOTS)),
                lambda p, e, t: p.swag_run(t["theta"], t["mean"], t["sq"], t["dev"], 2, e.x, e.y, e.tab, SIZES, LRS, 0, t["losses"]))

    @op("bbb_run")
    def _(r):
        return (dict(mu=w(r), rho=(-3.0 + 0.1 * r.normal(size=D)).astype(f32), w=blank(D), costs=blank(SLOTS, 4)),
                lambda p, e, t: p.bbb_run(t["mu"], t["rho"], t["w"], e.x, e.y, e.tab, SIZES, LRS, 0.1, 0.0, 0.5, 1, 9, t["costs"]))

    @op("adam_run")
    def _(r):
        return (dict(theta=w(r), m=w(r), v=pos(r), losses=blank(SLOTS)),
                lambda p, e, t: p.adam_run(t["theta"], t["m"], t["v"], e.x, e.y, e.tab, SIZES, LRS, (1, 1, 1, 2, 2), 0.9, 0.999,
                                           t["losses"]))

    @op("bsam_run")
    def _(r):
        return (dict(theta=w(r), m=w(r), v=pos(r), losses=blank(2 * SLOTS)),
                lambda p, e, t: p.bsam_run(t["theta"], t["m"], t["v"], e.x, e.y, e.tab, SIZES, LRS, 0.9, 0.999, 0.1, 0.05, 0.1,
                                           float(N_ROWS), 1, 5, t["losses"]))

    @op("sgld_chains_step")
    def _(r):
        return (dict(theta=w(r, P), mean=w(r, P), sq=pos(r, P), loss=blank(P)),
                lambda p, e, t: p.sgld_chains_step(t["theta"], t["mean"], t["sq"], e.x, e.y, 0.05, 3, 17, t["loss"],
                                                   batch=MAX_BATCH, row_idx=e.idx))

    @op("sgld_chains_run")
    def _(r):
        return (dict(theta=w(r, P), mean=w(r, P), sq=pos(r, P), losses=blank(SLOTS, P)),
                lambda p, e, t: p.sgld_chains_run(t["theta"], t["mean"], t["sq"], e.x, e.y, e.tab, SIZES, LRS, 3, 17, t["losses"]))

    @op("sgld_lanes_run")
    def _(r):
        rates = np.outer(np.asarray(LRS, dtype=f32), np.asarray((1.0, 0.5, 0.25), dtype=f32))
        return (dict(theta=w(r, P), mean=w(r, P), sq=pos(r, P), losses=blank(SLOTS, P)),
                lambda p, e, t: p.sgld_lanes_run(t["theta"], t["mean"], t["sq"], e.x, e.y, e.tab, SIZES, rates, 3, 17, t["losses"],
                                                 seed_stride=1))

    @op("lane_scores")
    def _(r):
        def fn(p, e, t):
            loss_sum, errors = p.lane_scores(t["weights"], e.x8, e.y8)
            return dict(loss_sum=loss_sum, errors=errors)
        return dict(weights=w(r, DRAWS)), fn

    def hmc_step(name, chains):
        @op(name)
        def _(r):
            q = w(r, chains) if chains > 1 else w(r)
            return (dict(q=q, stats=blank(chains, 8)),
                    lambda p, e, t: p.hmc_step(t["q"], e.x8, e.y8, 2, 0.01, 1.0, 0.0, 1.0, np.full(chains, 0.5, dtype=f32), 1, 3,
                                               t["stats"]))
    hmc_step("hmc_step_p1", 1)
    hmc_step("hmc_step_p3", P)

    @op("hmc_run_p1")
    def _(r):
        cap = N_STEPS + 1
        init = dict(q=w(r), stats_all=blank(SLOTS, 1, 8), samples=blank(1, cap, D), freq=np.zeros((1, cap), dtype=np.int32),
                    count=np.zeros(1, dtype=np.int32), fail=np.zeros(4, dtype=np.int32))
        us = np.full((N_STEPS, 1), 0.5, dtype=f32)
        return init, lambda p, e, t: p.hmc_run(t["q"], e.x8, e.y8, 2, 0.01, 1.0, 0.0, 1.0, us, 1, 1, 3, t["stats_all"],
                                               t["samples"], t["freq"], t["count"], t["fail"])

    def svgd_state(r):
        parts = w(r, P)
        return dict(parts=parts, snap=parts.copy(), am=(0.1 * w(r, P)).astype(f32), av=pos(r, P), loss=blank(1))

    @op("svgd_step")      # Gauss-Seidel: the whole particle matrix in place (the snapshot is the matrix itself)
    def _(r):
        return (svgd_state(r),
                lambda p, e, t: p.svgd_step(t["parts"], t["parts"], 0, t["am"], t["av"], e.x, e.y, 0.01, 1.0, 2, t["loss"],
                                            batch=MAX_BATCH, row_idx=e.idx))

    @op("svgd_grad_sweep")
    def _(r):
        def fn(p, e, t):
            p.svgd_gradients(t["parts"], e.x, e.y, batch=MAX_BATCH, row_idx=e.idx)
            p.svgd_sweep(t["parts"], t["snap"], 0, t["am"], t["av"], 0.01, 0.5, 2, t["loss"], sweep="jacobi")
        return svgd_state(r), fn

    @op("predict")
    def _(r):
        def fn(p, e, t):
            samples, mean = p.predict(t["weights"], e.x8)
            return dict(samples=samples, mean=mean)
        return dict(weights=w(r, DRAWS)), fn

    @op("predict_moments")
    def _(r):
        def fn(p, e, t):
            mean, m2 = p.predict_moments(t["weights"], e.x8)
            return dict(mean=mean, m2=m2)
        return dict(weights=w(r, DRAWS)), fn

    @op("predict_surface")
    def _(r):
        def fn(p, e, t):
            return dict(zip(("cols", "mean", "top", "cls", "ent"), p.predict_surface(t["weights"], e.x8, column=spec.dims[-1] - 1)))
        return dict(weights=w(r, DRAWS)), fn

    @op("input_grad")
    def _(r):
        def fn(p, e, t):
            return dict(zip(("xgrad", "xadv", "losses"), p.input_grad(t["weights"], e.x8, e.y8, scale=0.5, epsilon=0.1)))
        return dict(weights=w(r, DRAWS)), fn

    @op("fsvi_step")
    def _(r):
        init = dict(mu=w(r), parts=w(r, P), am=(0.1 * w(r)).astype(f32), av=pos(r), loss=blank(1),
                    lo=np.full(F, -2.0, dtype=f32), hi=np.full(F, 2.0, dtype=f32))
        return init, lambda p, e, t: p.fsvi_step(t["mu"], t["parts"], t["am"], t["av"], e.x, e.y, 4, 0.01, 1, 4, t["loss"],
                                                 lo=t["lo"], hi=t["hi"], batch=3, row_idx=e.idx)

    return B


def build_ops(env: Env, names=None) -> dict:
    """name -> allocated Op for every op of the spec's table (or for `names`), in table order."""
    builders = _builders(env.spec)
    names = TABLE[env.spec.name] if names is None else names
    assert set(names) <= set(builders), sorted(set(names) - set(builders))
    return {name: builders[name]().alloc(env) for name in names}


def op_names(spec_name: str) -> tuple:
    """The names build_ops would allocate (no device needed): the parametrisation of the GPU tests."""
    names = TABLE[spec_name]
    assert set(names) <= set(_builders(SPECS[spec_name])), "an op of the table has no builder"
    return names
