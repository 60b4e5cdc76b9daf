"""The case table of the device-resident SGD, SWAG, SGLD and BBB runs (pyz_sgd_run, pyz_swag_run, pyz_sgld_run, pyz_bbb_run:
all four are sgld_run_impl in csrc/pyz_api.hip) and the comparison both run tests share (a plain module).

A run adds to the step: step scalars that live on the device and ping-pong between two StepCtl slots (pyz_prepare_next), the
per-run tables (inline up to 32 steps, else through pinned staging buffers), batches assembled one step ahead by the idle
workgroups of the weight-gradient launch (pyz_prep_rows, pyz_copy_rows), graphs of 32 steps and a remainder graph by exact
length, SWAG's deviation row from the step count, BBB's next-step sample in the epilogue and its gated validation forward.
This module restates the host rules of sgld_run_impl and of what it shares with the other run entries: upload_run_tables
(`table_transport`, `first_batch_launch`) and the graph cache PyzGraphCache of pyz_common.h (`graph_chunks`); beside them
`batch_ahead`, `prep_partition` and `expected_run_launches`.  It names the cells of the coverage table (`CELLS`,
`reached_cells`, `book_cells`), lists cases that reach every cell with every mode they apply to, builds their data
(step_cases.step_data and a row table whose entries behind a step's batch are other valid rows), restates a run as a chain
of step_cases.ref_step (`ref_run_step`: learning rate and batch of step i, count n0 + i, row slot slot0 + i, the SWAG row,
the BBB gate) with the wrong variants the sensitivity check needs (`RUN_MUTATIONS`), and compares one step of a run through
step_cases.compare_step, unchanged (`compare_run_step`).  tests/test_run_dispatch_table.py pins all of it to the source
and to the oracle modules on the CPU; tests/test_gpu_run_matrix.py runs the cases on the device."""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import step_cases as sc
from dense_cases import can_fuse, cdiv, expected_launches, pick_waves, wgrad_steps, wgrad_tiles
from head_cases import expected_head_kernel
from oracle import bbb as o_bbb
from step_cases import MODES, SS, StepCase, StepData, compare_step, ref_step, step_data

# ---------------------------------------------------------------- the host rules (csrc/pyz_api.hip, pyz_kernels.h, pyz_fused.h)
INLINE_TAB = 32       # PYZ_INLINE_TAB: runs of at most this many steps carry their tables in a kernel's arguments
GRAPH_CHUNKS = 8      # PYZ_GRAPH_CHUNKS: slot 0 = a chunk of GRAPH_STEPS, seven slots for remainder graphs (LRU)
GRAPH_STEPS = 32      # default of PYZ_GRAPH_STEPS
CUS = 256             # compute units of the MI355X (pyz_cu_count)
AHEAD_SPARE = 24      # batch_ahead: wgrad tiles + 24 <= CUs; launch_wgrad_all: at least 24 batch workers
PREP_GRID = 256       # k_run_start / k_prep_batch: dim3(256) workgroups
GATE_MOD = 10         # BBB.py:203: the validation forward runs on steps with n % 10 != 0
ENV_FORBIDDEN = ("PYZ_GRAPH_STEPS", "PYZ_BATCH_AHEAD", "PYZ_BBB_FUSE_SAMPLE", "PYZ_GATHER_COPY", "PYZ_WAVES_TARGET",
                 "PYZ_MIN_STEPS", "PYZ_FWD_KSPLIT")
N_STEPS = 6           # the short ragged run
LR_FACTORS = (1.0, 0.75, 0.875, 0.5, 0.625, 0.375)   # learning rate of step i over the case's: every neighbour differs


def table_transport(n_steps: int) -> str:
    """upload_run_tables: `if (n_steps <= PYZ_INLINE_TAB)` the tables ride in k_run_start / k_set_ctl_tabs, else they go up
    through one of the two pinned staging buffers."""
    return "inline" if n_steps <= INLINE_TAB else "pinned"


def wgrad_tile_count(dims) -> int:
    return sum(wgrad_tiles(K, N) for K, N in zip(dims[:-1], dims[1:]))


def batch_ahead(dims) -> bool:
    """batch_ahead (PYZ_BATCH_AHEAD at its default 1): fused path, a hidden layer, and tiles + 24 <= CUs."""
    return can_fuse(dims) and len(dims) - 1 > 1 and wgrad_tile_count(dims) + AHEAD_SPARE <= CUS


def first_batch_launch(dims, n_steps: int) -> Optional[str]:
    """Who assembles the first batch of a run: k_run_start together with the inline tables, else k_prep_batch."""
    if not batch_ahead(dims):
        return None
    return "k_run_start" if table_transport(n_steps) == "inline" else "k_prep_batch"


def graph_chunks(n_steps: int):
    """Lengths of the graphs a run launches: chunks of GRAPH_STEPS and one remainder graph of the exact length."""
    out = [GRAPH_STEPS] * (n_steps // GRAPH_STEPS)
    return out + ([n_steps % GRAPH_STEPS] if n_steps % GRAPH_STEPS else [])


def epilogue_workers(dims) -> int:
    """launch_wgrad_all: grid.x = tiles + 1 + max(CUs - tiles - 1, 24) when a batch is prepared."""
    return max(CUS - wgrad_tile_count(dims) - 1, AHEAD_SPARE)


def fwd_tile_grid(dims, bmax: int):
    """prep_args: (fwd_tiles, fwd_tiles_n) of the forward launch that reads the assembled batch (grid of `bmax` rows)."""
    tn = cdiv(dims[1], 32)
    return cdiv(bmax, 32) * tn, tn


def prep_partition(nb: int, cnt: int, first_id: int, fwd_tiles: int, fwd_tiles_n: int):
    """pyz_prep_rows for every worker j of cnt (workgroup id first_id + j): [(ra, rb)] of the nb rows, and per residue of the
    XCD-aware branch its (r0, r1) (empty list on the simple branch)."""
    out, residues = [], []
    xcd = cnt >= 8 and fwd_tiles >= 8
    for j in range(cnt):
        bid = first_id + j
        if xcd:
            x, q, r = bid & 7, fwd_tiles >> 3, fwd_tiles & 7
            t0 = x * (q + 1) if x < r else r * (q + 1) + (x - r) * q
            t1 = t0 + (q + 1 if x < r else q)
            b0, b1 = cdiv(t0, fwd_tiles_n), cdiv(t1, fwd_tiles_n)
            r0, r1 = min(32 * b0, nb), (nb if x == 7 else min(32 * b1, nb))
            id0 = bid - j
            first = id0 + ((x - (id0 & 7)) & 7)
            mine, everyone = (bid - first) >> 3, (id0 + cnt - 1 - first) // 8 + 1
            per = cdiv(r1 - r0, everyone)
            ra = r0 + mine * per
            rb = min(ra + per, r1)
            if j < 8:
                residues.append((r0, r1))
        else:
            per = cdiv(nb, cnt)
            ra = j * per
            rb = min(ra + per, nb)
        out.append((ra, rb))
    return out, residues


def loss_nblk(max_batch: int, grid_batch: int) -> int:
    """pyz_api.hip loss_nblk: partial sums of the unfused loss kernels (256 rows each)."""
    return min(cdiv(max_batch, 256), cdiv(grid_batch, 256))


# ---------------------------------------------------------------- cases
class RunCall(NamedTuple):
    """One call of a run entry point."""
    n0: int                  # step count of its first step (SGLD / SWAG: n0; BBB: step0; SGD: unused)
    slot0: int               # row-table / loss slot of its first step
    sizes: tuple             # batch size per step
    lrs: tuple               # learning rate per step
    k: int = 0               # SWAG: rows of the deviation matrix
    freq: int = 0            # SWAG: moments / deviation on steps with n % freq == 0
    val: bool = False        # BBB: with the validation forward


class RunCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str
    bmax: int
    sizes: tuple             # the short ragged run: the largest batch first, so every prefix launches for bmax
    modes: tuple = MODES
    aligned: bool = False
    prior_vec: bool = False
    lr: float = 0.5
    bbb_lr: float = 0.5
    n0: int = 3
    slot0: int = 2
    seed: int = 11
    swag: tuple = (3, 2)     # (k, frequency) of the short run: n0 = 3 gives hits at steps 1, 3 and 5, rows 2, 2, 2
    data_seed: int = 0

    @property
    def step(self) -> StepCase:
        """The step case of this shape at its largest batch (gathered: x holds more rows than a batch)."""
        return StepCase(self.name, self.dims, self.acts, self.loss, self.bmax, True, self.lr, self.bbb_lr, self.n0,
                        seed=self.seed, prior_vec=self.prior_vec, aligned=self.aligned, data_seed=self.data_seed)

    @property
    def spec(self):
        return self.step.spec

    @property
    def D(self) -> int:
        return self.step.D

    @property
    def fused(self) -> bool:
        return can_fuse(self.dims)

    @property
    def max_batch(self) -> int:
        """row_stride of the runs: different from bmax in every case."""
        return self.bmax + 3

    @property
    def ahead(self) -> bool:
        return batch_ahead(self.dims)

    @property
    def S(self) -> int:
        """Waves of the chained k_wgrad_all: picked from bmax whatever the step's own batch (0 when unfused)."""
        return pick_waves(wgrad_tile_count(self.dims), wgrad_steps(self.bmax))[0] if self.fused else 0

    def call(self, mode: str, n_steps: int = N_STEPS, val: bool = False) -> RunCall:
        """The first n_steps of the short ragged run."""
        lr = self.bbb_lr if mode == "bbb" else self.lr
        k, freq = self.swag if mode == "swag" else (0, 0)
        return RunCall(self.n0, self.slot0, self.sizes[:n_steps], tuple(lr * f for f in LR_FACTORS[:n_steps]), k, freq, val)


R, T, G, LN, SM = "relu", "tanh", "sigmoid", "linear", "softmax"
SC, MS = "scce", "mse"


def _c(name, dims, acts, loss, bmax, sizes, **kw):
    assert sizes[0] == bmax == max(sizes) and len(sizes) == N_STEPS
    return RunCase(name, tuple(dims), tuple(acts), loss, bmax, tuple(sizes), **kw)


CASES = [
    _c("r_s4", (24, 16, 4), (R, SM), SC, 64, (64, 23, 64, 1, 7, 64), aligned=True, swag=(3, 1), bbb_lr=0.25),
    _c("r_s4_scalar_copy", (23, 16, 4), (R, SM), SC, 64, (64, 22, 64, 1, 5, 33), prior_vec=True, bbb_lr=0.25),
    _c("r_s2", (31, 20, 10), (T, SM), SC, 45, (45, 3, 45, 1, 17, 44)),
    _c("r_s1", (20, 16, 4), (R, SM), SC, 14, (14, 1, 14, 5, 9, 14), aligned=True, prior_vec=True, bbb_lr=0.25),
    _c("r_s4_xcd12", (16, 70, 10), (T, SM), SC, 97, (97, 33, 97, 1, 7, 64), swag=(1, 2)),
    _c("r_s8_xcd8_l3_mse", (20, 64, 31, 6), (G, T, LN), MS, 128, (128, 89, 128, 1, 15, 33), prior_vec=True, bbb_lr=0.25),
    _c("r_s16_xcd24", (20, 96, 10), (R, SM), SC, 256, (256, 89, 256, 1, 31, 256), aligned=True, bbb_lr=0.25),
    _c("r_l1", (31, 10), (SM,), SC, 63, (63, 22, 63, 1, 7, 40)),
    _c("r_unfused_d1100", (12, 20, 40), (T, SM), SC, 70, (70, 23, 70, 1, 7, 64), modes=("sgld",), data_seed=2),
    _c("r_unfused_d218", (3, 5, 33), (T, SM), SC, 300, (300, 256, 300, 1, 77, 257), modes=("sgld",), aligned=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"
FUSED_CASES = [c for c in CASES if c.fused]
UNFUSED_CASES = [c for c in CASES if not c.fused]

CHAIN_COUNTS = (32, 33, 70)            # fused cases, as two calls: n // 2 and the rest
CHAIN_COUNTS_UNFUSED = (6, 33)


class Book(NamedTuple):
    """A SWAG or BBB bookkeeping run (tests/test_gpu_run_matrix.py runs it with the oracle tier's method)."""
    name: str
    mode: str
    case: str
    n0: int
    n_steps: int
    k: int = 0
    freq: int = 0
    before: int = 0          # SWAG: steps of an earlier call that ends at n0 (the run continues its state and slots)
    val: bool = False


BOOKS = [
    Book("swag_first_hit_cap", "swag", "r_s4", 0, 6, k=3, freq=1),            # rows 0, 1, 2, 2, 2, 2
    Book("swag_k1", "swag", "r_s4_scalar_copy", 0, 4, k=1, freq=2),           # row 0 at n = 0 and 2
    Book("swag_continued", "swag", "r_s2", 4, 6, k=4, freq=3, before=4),      # rows 0, 1 before; 2 (n = 6), 3 (n = 9) now
    Book("swag_no_hit", "swag", "r_s1", 1, 4, k=3, freq=5),                   # n = 1 .. 4: nothing but theta moves
    Book("bbb_gate_first_odd", "bbb", "r_s4", 10, 5, val=True),
    Book("bbb_gate_last_even", "bbb", "r_s4_scalar_copy", 5, 6, val=True),
    Book("bbb_gate_on_chunk_boundary", "bbb", "r_s1", 8, 34, val=True),       # step 32 of the call has n = 40
]
N_VAL = 37                # rows of the validation split (n_val % 32 != 0)
VAL_MAX_BATCH = 40        # max_batch of the validation plan: another one than any case's


def book_call(book: Book) -> tuple:
    """(case, the calls of a bookkeeping run in order): batches cycle through the case's ragged sizes, the one-row batch
    replaced by a whole one."""
    case = CASE_BY_NAME[book.case]
    lr = case.bbb_lr if book.mode == "bbb" else case.lr
    ragged = tuple(case.bmax if b == 1 else b for b in case.sizes)   # (a one-row batch can have a loss float32 cannot resolve to 1e-4)
    sizes = lambda n, o=0: tuple(ragged[(o + i) % N_STEPS] for i in range(n))
    lrs = lambda n, o=0: tuple(lr * LR_FACTORS[(o + i) % N_STEPS] for i in range(n))
    calls = []
    if book.before:
        calls.append(RunCall(book.n0 - book.before, 1, (case.bmax,) + sizes(book.before - 1, 1), lrs(book.before), book.k, book.freq))
    slot0 = 1 + book.before
    calls.append(RunCall(book.n0, slot0, sizes(book.n_steps), lrs(book.n_steps), book.k, book.freq, book.val))
    return case, calls


# ---------------------------------------------------------------- the launches of an eager-chained run
def _norm(name: str) -> str:
    return name.replace(" ", "").strip("()")


def expected_run_launches(case: RunCase, mode: str, n_steps: int, n_val: int = 0) -> list:
    """Every launch of one eager-chained run (use_graph off, or inside KernelProbe) in order, spaces removed.
    sgld_run_impl: [k_set_ctl of the validation plan], then upload_run_tables: k_run_start | k_set_ctl_tabs (inline
    tables) or k_set_ctl [+ k_prep_batch] (pinned tables); per step launch_sgld_step at grid batch bmax: BBB's k_bbb_sample on the first step
    only (later weights come out of the epilogue before), hidden forwards, head, hidden data gradients, k_wgrad_all<S>;
    BBB with validation: hidden forwards, head and k_loss_finalize_gated of the validation plan, in every step; unfused
    SGLD: every forward, the loss kernel, data / weight gradients per layer from the last, k_sgld_update."""
    dims, L = case.dims, len(case.dims) - 1
    out = []
    if n_val:
        out.append("k_set_ctl")
    if table_transport(n_steps) == "inline":
        out.append("k_run_start" if case.ahead else "k_set_ctl_tabs")
    else:
        out.append("k_set_ctl")
        if case.ahead:
            out.append("k_prep_batch")
    la = expected_launches(case.step.dense)
    for i in range(n_steps):
        if case.fused:
            if mode == "bbb" and i == 0:
                out.append("k_bbb_sample")
            out += [f.kernel for f in la.fwd]
            out.append(expected_head_kernel(dims, case.loss, 1, case.bmax))
            out += ["k_dense_bwd_data"] * len(la.bwd_data)
            out += [w.kernel for w in la.wgrad]
            if n_val:
                out += ["k_dense_fwd"] * (L - 1) + [expected_head_kernel(dims, case.loss, 1, n_val), "k_loss_finalize_gated"]
        else:
            assert mode == "sgld"
            out += ["k_dense_fwd"] * L + ["k_loss_scce" if case.loss == "scce" else "k_loss_mse"]
            for l in range(L - 1, -1, -1):
                out += (["k_dense_bwd_data"] if l > 0 else []) + ["k_dense_bwd_weight"]
            out.append("k_sgld_update")
    return [_norm(n) for n in out]


def expected_run_path(n_steps: int, use_graph: bool, side_stream: bool):
    """(last_run_path(), last_run_graph_launches()): graphs need use_graph and a stream of the caller's own."""
    if use_graph and side_stream:
        return ("graph", n_steps), len(graph_chunks(n_steps))
    return ("eager", n_steps), 0


# ---------------------------------------------------------------- the coverage table
CELLS = frozenset(
    [f"{m} chained S={S} batch below bmax" for m in MODES for S in SS] +
    [f"S={S} {b}" for S in SS for b in ("batch 1", "odd batch", "batch below 2S")] +
    ["prep simple branch", "prep XCD branch fwd_tiles&7==0", "prep XCD branch fwd_tiles&7!=0", "fwd_tiles == 8",
     "more than one forward column tile", "XCD residue without tiles", "XCD residue emptied by a small batch",
     "copy 16-byte loop", "copy scalar loop", "first batch by k_run_start", "first batch by k_prep_batch",
     "no batch-ahead: one layer", "no batch-ahead: unfused",
     "unfused chained SGLD D%4!=0", "unfused chained SGLD D>1024", "unfused chained SGLD loss_nblk>=2, then a step of <=256 rows",
     "SWAG hit on the first step of a call", "SWAG n0>0 continued from an earlier call", "SWAG row capped at k-1 and replaced twice",
     "SWAG k=1", "SWAG frequency 1", "SWAG frequency >1", "SWAG call with no hit",
     "BBB odd step count", "BBB even step count", "BBB chunk boundary inside the run", "BBB prior vectors",
     "BBB validation n_val%32!=0 on a plan of another max_batch", "BBB gated step first", "BBB gated step last",
     "BBB gated step on a chunk boundary", "slot0 > 0", "state buffers 4 bytes off 16-byte alignment",
     "state buffers 16-byte aligned"])


def swag_row(n: int, k: int, freq: int) -> int:
    """pyz_update_math: min((nstep + swag_freq - 1) / swag_freq, swag_k - 1)."""
    return min(cdiv(n, freq), k - 1)


def reached_cells(case: RunCase) -> set:
    """The cells a case reaches with its modes in the oracle tier (the short ragged run and its prefixes) and the chain
    tier (CHAIN_COUNTS), from its shape and the restated rules alone."""
    cells = set()
    later = case.sizes[1:]
    if case.fused:
        S = case.S
        if any(b < case.bmax for b in later):
            cells |= {f"{m} chained S={S} batch below bmax" for m in case.modes}
        if 1 in later:
            cells.add(f"S={S} batch 1")
        if any(b % 2 and b > 1 for b in later):
            cells.add(f"S={S} odd batch")
        if any(b < 2 * S for b in later):
            cells.add(f"S={S} batch below 2S")
    if case.ahead:
        ft, tn = fwd_tile_grid(case.dims, case.bmax)
        grids = ((PREP_GRID, 0), (epilogue_workers(case.dims), wgrad_tile_count(case.dims) + 1))
        if ft >= 8:
            cells.add("prep XCD branch fwd_tiles&7==0" if ft % 8 == 0 else "prep XCD branch fwd_tiles&7!=0")
            if ft == 8:
                cells.add("fwd_tiles == 8")
            for nb in set(case.sizes):
                for cnt, first in grids:
                    _, res = prep_partition(nb, cnt, first, ft, tn)
                    _, full = prep_partition(case.bmax, cnt, first, ft, tn)
                    for (r0, r1), (f0, f1) in zip(res, full):
                        if f0 == f1:
                            cells.add("XCD residue without tiles")
                        elif r0 == r1:
                            cells.add("XCD residue emptied by a small batch")
        else:
            cells.add("prep simple branch")
        if tn > 1:
            cells.add("more than one forward column tile")
        cells.add("copy 16-byte loop" if case.dims[0] % 4 == 0 else "copy scalar loop")
        cells |= {"first batch by k_run_start", "first batch by k_prep_batch"}   # prefixes of 1 .. 6 steps; 33 and 70 steps
    elif case.fused:
        cells.add("no batch-ahead: one layer")
    else:
        cells.add("no batch-ahead: unfused")
        if case.D % 4:
            cells.add("unfused chained SGLD D%4!=0")
        if case.D > 1024:
            cells.add("unfused chained SGLD D>1024")
        if loss_nblk(case.max_batch, case.bmax) >= 2 and any(b <= 256 for b in later):
            cells.add("unfused chained SGLD loss_nblk>=2, then a step of <=256 rows")
    if "bbb" in case.modes:
        cells |= {"BBB odd step count", "BBB even step count", "BBB chunk boundary inside the run"}   # prefixes; 33 and 70 steps
        if case.prior_vec:
            cells.add("BBB prior vectors")
    if "swag" in case.modes:
        cells.add("SWAG frequency 1" if case.swag[1] == 1 else "SWAG frequency >1")
    if case.slot0 > 0:
        cells.add("slot0 > 0")
    cells.add("state buffers 16-byte aligned" if case.aligned else "state buffers 4 bytes off 16-byte alignment")
    return cells & CELLS


def book_cells(book: Book) -> set:
    """The cells a bookkeeping run reaches, from its step counts alone."""
    cells = set()
    case, calls = book_call(book)
    call = calls[-1]
    ns = [call.n0 + i for i in range(book.n_steps)]
    if book.mode == "swag":
        hits = [n for n in ns if n % book.freq == 0]
        rows = [swag_row(n, book.k, book.freq) for n in hits]
        if ns[0] % book.freq == 0:
            cells.add("SWAG hit on the first step of a call")
        if book.before and book.n0 > 0 and hits:
            cells.add("SWAG n0>0 continued from an earlier call")
        if book.k > 1 and sum(r == book.k - 1 and cdiv(n, book.freq) > book.k - 1 for r, n in zip(rows, hits)) >= 2:
            cells.add("SWAG row capped at k-1 and replaced twice")
        if book.k == 1 and hits:
            cells.add("SWAG k=1")
        if not hits:
            cells.add("SWAG call with no hit")
        cells.add("SWAG frequency 1" if book.freq == 1 else "SWAG frequency >1")
    else:
        gated = [i for i, n in enumerate(ns) if n % GATE_MOD == 0]
        cells.add("BBB odd step count" if book.n_steps % 2 else "BBB even step count")
        if book.n_steps > GRAPH_STEPS:
            cells.add("BBB chunk boundary inside the run")
        if book.val:
            assert N_VAL % 32 and VAL_MAX_BATCH != case.max_batch
            cells.add("BBB validation n_val%32!=0 on a plan of another max_batch")
            if 0 in gated:
                cells.add("BBB gated step first")
            if book.n_steps - 1 in gated:
                cells.add("BBB gated step last")
            if any(i and i % GRAPH_STEPS == 0 for i in gated):
                cells.add("BBB gated step on a chunk boundary")
    return cells & CELLS


def old_run_shapes():
    """The shapes the older run tests use, as cases of this table (for judging what they reach): name -> RunCase.  All have
    aligned fresh buffers, max_batch equal to the largest batch, slot0 = 0 in the first call and scalar priors."""
    t = lambda name, dims, acts, loss, bmax, small, modes: RunCase(name, dims, acts, loss, bmax, (bmax, bmax, small) * 2, modes,
                                                                   aligned=True, slot0=0)
    return {
        "test_gpu_batch_ahead.py::test_sgld_run_equals_eager_steps[24]": t("ba24", (24, 16, 4), (R, SM), SC, 64, 22, ("sgld",)),
        "test_gpu_batch_ahead.py::test_sgld_run_equals_eager_steps[23]": t("ba23", (23, 16, 4), (R, SM), SC, 64, 22, ("sgld",)),
        "test_gpu_batch_ahead.py::test_sgd_run_with_float_targets_equals_eager_steps": t("ba_mse", (6, 8, 2), (T, LN), MS, 32, 32, ("sgd",)),
        "test_gpu_bbb_run.py::test_bbb_run_equals_eager_steps": t("bbb", (24, 32, 16, 5), (R, T, SM), SC, 64, 52, ("bbb",)),
        "test_gpu_bbb_run.py::test_bbb_run_first_steps_match_the_oracle": t("bbb3", (12, 20, 4), (R, SM), SC, 32, 32, ("bbb",)),
        "test_gpu_baseline_shapes.py (784-200-10, batch 1000)": t("c2", (784, 200, 10), (R, SM), SC, 1000, 1000, ("sgld", "bbb")),
    }


# ---------------------------------------------------------------- data
class RunData(NamedTuple):
    step: StepData           # x, y, theta0, mean0, sq0, dev0 (2 rows), rho0, prior vectors (rows / ys: of the first bmax-batch)
    tab: np.ndarray          # (slots, max_batch) int32: every entry a valid row, the ones behind a step's batch included
    dev0: np.ndarray         # (8, D): starting deviation rows (a run takes the first k)
    xv: np.ndarray           # the validation split (N_VAL rows of their own)
    yv: np.ndarray


def run_data(case: RunCase, slots: int = 80) -> RunData:
    """step_cases.step_data of the case at bmax (non-zero starting state, edges weighted) and a row table: slot s holds the
    first max_batch entries of a permutation of all rows of x, so the entries behind a step's batch are valid but OTHER rows
    -- a kernel that reads past `batch` changes the result instead of faulting."""
    d = step_data(case.step)
    rng = np.random.default_rng(4001 + sum(map(ord, case.name)))
    n_rows = d.x.shape[0]
    assert n_rows >= case.max_batch
    tab = np.stack([rng.permutation(n_rows)[:case.max_batch] for _ in range(slots)]).astype(np.int32)
    dev0 = rng.normal(size=(8, case.D)).astype(np.float32)
    xv = rng.normal(size=(N_VAL, case.dims[0])).astype(np.float32)
    yv = (rng.integers(0, case.dims[-1], size=N_VAL).astype(np.int32) if case.loss == "scce"
          else rng.normal(size=(N_VAL, case.dims[-1])).astype(np.float32))
    return RunData(d, tab, dev0, xv, yv)


def initial_state(mode: str, data: RunData, k: int = 0) -> dict:
    s = sc.initial_state(mode, data.step)
    if mode == "swag":
        s["dev"] = data.dev0[:k].copy()
    return s


# ---------------------------------------------------------------- a run as a chain of ref_step, with the wrong variants
RUN_MUTATIONS = {   # name -> the modes it applies to
    "lr of step i+1 used at step i": MODES,
    "step count not advanced": ("swag", "sgld", "bbb"),
    "row offset advanced by bmax instead of max_batch": MODES,
    "batch taken as bmax (padding rows included)": MODES,
    "loss slot without slot0": MODES,
    "SWAG row by floor instead of ceil": ("swag",),
    "SWAG hit tested on n+1": ("swag",),
    "BBB Philox step i instead of step0 + i": ("bbb",),
    "BBB gate inverted": ("bbb",),
    "BBB prior vector ignored": ("bbb",),
}
# At a hit n is a multiple of the frequency, so floor(n / f) and ceil(n / f) are the same row: this wrong reference is the
# right one, bit for bit, on every input (tests/test_run_dispatch_table.py asserts exactly that and pins the row expression
# to the source text instead).
EQUIVALENT_MUTATIONS = ("SWAG row by floor instead of ceil",)


def run_mutation_applies(case: RunCase, call: RunCall, mode: str, mutation: str) -> bool:
    if mode not in RUN_MUTATIONS[mutation] or mutation in EQUIVALENT_MUTATIONS:
        return False
    if mutation == "loss slot without slot0":
        return call.slot0 > 0
    if mutation == "batch taken as bmax (padding rows included)":
        return any(b < case.bmax for b in call.sizes)
    if mutation == "SWAG hit tested on n+1":
        return call.freq > 1
    if mutation == "BBB Philox step i instead of step0 + i":
        return call.n0 > 0
    if mutation == "BBB gate inverted":
        return call.val
    if mutation == "BBB prior vector ignored":
        return case.prior_vec
    if mutation == "step count not advanced" and mode == "swag":      # without a hit, now or then, a SWAG step never reads n
        return any((call.n0 + i) % call.freq == 0 for i in range(1, len(call.sizes))) or (len(call.sizes) > 1 and call.n0 % call.freq == 0)
    return len(call.sizes) > 1


class StepView(NamedTuple):
    case: StepCase           # the step case whose step k is step i of the run
    k: int                   # index into step_cases.SWAG_STEPS: 0 = an update into row 1 of two, 1 = no update
    data: StepData
    hit: bool                # SWAG: moments and a deviation row are written
    row: int                 # SWAG: the row
    n: int
    slot: int
    validates: bool          # BBB with validation: n % 10 != 0


def step_view(case: RunCase, data: RunData, call: RunCall, mode: str, i: int, mutation=None) -> StepView:
    """Step i of a call as step_cases sees one step: the chain rules of pyz_prepare_next and pyz_update_math."""
    n, lr, b = call.n0 + i, call.lrs[i], call.sizes[i]
    off, slot = (call.slot0 + i) * case.max_batch, call.slot0 + i
    if mutation == "lr of step i+1 used at step i":
        lr = call.lrs[min(i + 1, len(call.lrs) - 1)]
    if mutation == "step count not advanced":
        n = call.n0
    if mutation == "row offset advanced by bmax instead of max_batch":
        off = call.slot0 * case.max_batch + i * case.bmax
    if mutation == "batch taken as bmax (padding rows included)":
        b = case.bmax
    if mutation == "loss slot without slot0":
        slot = i
    rows = data.tab.reshape(-1)[off:off + b]
    hit, row, k, n_view = True, 0, 0, n
    if mode == "swag":
        hit = ((n + 1) if mutation == "SWAG hit tested on n+1" else n) % call.freq == 0
        row = min(n // call.freq, call.k - 1) if mutation == "SWAG row by floor instead of ceil" else swag_row(n, call.k, call.freq)
        if not hit:
            k, n_view = 1, n - 1          # SWAG_STEPS[1]: no update (step_cases counts n0 + k)
    if mode == "bbb" and mutation == "BBB Philox step i instead of step0 + i":
        n_view = i
    validates = bool(call.val) and ((n % GATE_MOD == 0) if mutation == "BBB gate inverted" else (n % GATE_MOD != 0))
    view = case.step._replace(batch=int(b), lr=lr, bbb_lr=lr, n0=n_view)
    d = data.step._replace(rows=data.step.x[rows], ys=data.step.y[rows], idx=rows)
    return StepView(view, k, d, hit, row, n, slot, validates)


def _two_rows(dev, row):
    """The deviation matrix as step_cases' two rows: [some other row (or zeros), the row this step may write]."""
    other = dev[(row + 1) % dev.shape[0]] if dev.shape[0] > 1 else np.zeros_like(dev[0])
    return np.stack([other, dev[row]])


def ref_run_step(case: RunCase, data: RunData, call: RunCall, mode: str, i: int, s0: dict, dtype=np.float64, mutation=None) -> dict:
    """Step i of the call from the state s0 in `dtype` (device noise: the Philox draws of count n0 + i): the new state, the
    loss (BBB: cost, kl_abs), "slot" = where the loss lands, and for BBB with validation "val" = the validation loss of the
    sampled weights or None on a gated step."""
    v = step_view(case, data, call, mode, i, mutation)
    variant = "device" if mode in sc.STREAM else "plain"
    s0v = dict(s0)
    if mode == "swag":
        s0v["dev"] = _two_rows(np.asarray(s0["dev"], dtype=dtype), v.row)
    out = ref_step(v.case, v.data, mode, variant, v.k, s0v, dtype, mutation if mutation in sc.MUTATIONS else None)
    if mode == "swag":
        dev = np.asarray(s0["dev"], dtype=dtype).copy()
        dev[v.row] = out["dev"][1]
        out["dev"] = dev
    out["slot"] = v.slot
    if mode == "bbb" and call.val:
        out["val"] = o_bbb.validation_loss(out["w"], data.xv, data.yv, case.spec, dtype) if v.validates else None
    return out


def compare_run_step(case: RunCase, data: RunData, call: RunCall, mode: str, i: int, s0: dict, got: dict, ref: dict, what: str = "") -> dict:
    """One step of a run: `got` (float32 state after it, loss or cost triple, the slot it was found in, validation loss or
    None) against the float64 reference `ref` of the same step from the same state s0, through step_cases.compare_step
    unchanged; the deviation rows the step does not own, the slot and the gate exactly; a validation loss like a loss (1e-4
    relative).  Returns quantity -> error over tolerance."""
    v = step_view(case, data, call, mode, i)
    what = f"{what}run step {i} (n = {v.n}, batch {v.case.batch}): "
    s0v, gotv, refv = dict(s0), dict(got), dict(ref)
    if mode == "swag":
        for d in (s0v, gotv, refv):
            d["dev"] = _two_rows(np.asarray(d["dev"]), v.row)
    rep = compare_step(v.case, mode, v.k, s0v, gotv, refv, what=what)
    if mode == "swag":
        for r in range(call.k):
            if not (v.hit and r == v.row):
                sc._same_bits(got["dev"][r], s0["dev"][r], f"{what}{case.name}: deviation row {r}, which this step does not write")
    assert got["slot"] == ref["slot"] == v.slot, f"{what}{case.name} {mode}: loss found in slot {got['slot']}, expected {v.slot}"
    if mode == "bbb" and call.val:
        assert (got["val"] is None) == (ref["val"] is None) == (not v.validates), \
            f"{what}{case.name}: validation {'ran' if got['val'] is not None else 'did not run'} at n = {v.n}"
        if v.validates:
            rep["val"] = sc._ratio(abs(float(got["val"]) - float(ref["val"])), 1e-4 * abs(float(ref["val"])))
            assert rep["val"] <= 1.0, f"{what}{case.name}: validation loss {got['val']!r} against {ref['val']!r}"
    return rep


def stored(out: dict) -> dict:
    """What a float32 device would leave of a reference step."""
    keep = {k: v for k, v in out.items() if k not in ("slot", "val")}
    s = sc.as_stored(keep)
    s["slot"] = out["slot"]
    if "val" in out:
        s["val"] = None if out["val"] is None else np.float32(out["val"])
    return s


def next_state(s0: dict, out: dict) -> dict:
    return {k: out[k] for k in s0}
