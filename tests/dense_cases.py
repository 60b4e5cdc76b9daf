"""The Dense GEMM case table and the launch rules it relies on (a plain module: imported by the dense tests).

Every Dense kernel is a family whose member is picked from the shape at launch.  This module restates those launch
decisions in plain Python (each with its source location), derives from them which kernel, wave count S and operand path
a case runs (`expected_launches`), names the cells of the coverage table (`CELLS`, `reached_cells`) and lists cases that
together reach every cell.  tests/test_dense_dispatch_table.py pins the restatement to the source on the CPU;
tests/test_gpu_dense_matrix.py runs the cases against the float64 oracle."""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from oracle import mlp as o_mlp

# ---------------------------------------------------------------- launch rules (csrc/pyz_gemm.h unless noted)
WAVES_TARGET = 3072      # pyz_pick_waves: default of PYZ_WAVES_TARGET (read once per process)
MIN_STEPS = 8            # pyz_pick_waves: default of PYZ_MIN_STEPS (read once per process)
LDS_MAXROWS = 2048       # pyz_fwd_takes_lds: default of PYZ_FWD_LDS_MAXROWS
LDS_MINWG = 256          # pyz_fwd_takes_lds: default of PYZ_FWD_LDS_MINWG (read per call)
LDS_MIN_N, LDS_MIN_ROWS, LDS_MANY_P = 48, 128, 8   # pyz_fwd_takes_lds: g.N >= 48, grid_batch >= 128, P >= 8
LDS_NT_N = (64, 128)     # pyz_fwd_takes_lds / pyz_launch_fwd: NT = 2 up to 64 columns, 4 up to 128, else 7
RING_MINWG, RING_MAXWG = 192, 1024   # pyz_gemm_ring.h, pyz_fwd_ring_variant: PYZ_FWD_RING_MINWG / _MAXWG
RING_N = (192, 200)      # pyz_fwd_ring_variant: 192 < N <= 200
FUSE_MAX_N = 32          # pyz_api.hip, can_fuse: last layer of at most 32 units
WGRAD_ALL_S = (1, 2, 4, 8, 16)       # pyz_api.hip, launch_wgrad_all: the arms of switch (S) (default: 16)
ENV_FORBIDDEN = ("PYZ_WAVES_TARGET", "PYZ_MIN_STEPS", "PYZ_GATHER_COPY")   # read once per process: left alone


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def pick_waves(tiles: int, mfma_steps: int):
    """pyz_pick_waves: (S, exit) with exit = which condition ended the doubling: "steps" (a wave would get fewer than
    MIN_STEPS steps), "tiles" (tiles x S reached the target) or "cap" (S = 16)."""
    S = 1
    while S < 16 and tiles * S < WAVES_TARGET and mfma_steps // (2 * S) >= MIN_STEPS:
        S *= 2
    if S == 16:
        return S, "cap"
    return S, "tiles" if tiles * S >= WAVES_TARGET else "steps"


def pad8(n: int, P: int) -> int:
    """pyz_pad8: grid.x in multiples of 8 when the launch has several particles."""
    return cdiv(n, 8) * 8 if P > 1 else n


def fwd_steps(K: int) -> int:          # pyz_launch_fwd: pyz_pick_waves(tiles * P, (g.K + 1) / 2 + 1)
    return (K + 1) // 2 + 1


def bwd_data_steps(N: int) -> int:     # pyz_launch_bwd_data: pyz_pick_waves(tiles * P, (g.N + 1) / 2)
    return (N + 1) // 2


def wgrad_steps(batch: int) -> int:    # pyz_launch_bwd_weight and pyz_api.hip launch_wgrad_all: (grid_batch + 1) / 2
    return (batch + 1) // 2


def fwd_tiles(batch: int, N: int) -> int:        # pyz_launch_fwd
    return cdiv(batch, 32) * cdiv(N, 32)


def bwd_data_tiles(batch: int, K: int) -> int:   # pyz_launch_bwd_data
    return cdiv(batch, 32) * cdiv(K, 32)


def wgrad_tiles(K: int, N: int) -> int:          # pyz_launch_bwd_weight; summed over layers in pyz_api.hip wgrad_layers
    return cdiv(K + 1, 32) * cdiv(N, 32)


def can_fuse(dims) -> bool:            # pyz_api.hip can_fuse
    return dims[-1] <= FUSE_MAX_N


def w_offsets(dims):
    """Offset of each layer's [W; b] block in the flat vector (m->w_off)."""
    out, off = [], 0
    for K, N in zip(dims[:-1], dims[1:]):
        out.append(off)
        off += (K + 1) * N
    return out


def fwd_vec(K: int, in_aligned16: bool) -> int:  # pyz_api.hip forward_args: (g.K % 8 == 0) && aligned16(g.in)
    return int(K % 8 == 0 and in_aligned16)


def bwd_data_vec(N: int, w_off: int, P: int, D: int) -> int:
    """pyz_api.hip launch_backward / launch_bwd_data_hidden: N % 8 == 0, w_off % 4 == 0, particle stride % 4 == 0 (the
    parameter tensor itself is 16-byte aligned: a fresh device allocation)."""
    return int(N % 8 == 0 and w_off % 4 == 0 and (P == 1 or D % 4 == 0))


def lds_nt(N: int) -> int:
    return 2 if N <= LDS_NT_N[0] else 4 if N <= LDS_NT_N[1] else 7


def fwd_takes_lds(K, N, batch, P, D, w_off, S, in_aligned16, lds_on=1, min_wg=LDS_MINWG):
    """pyz_fwd_takes_lds (no gate; the activations, the parameters and the batch copy are fresh device allocations)."""
    lds_ok = K % 4 == 0 and N % 2 == 0 and w_off % 2 == 0 and (P == 1 or D % 2 == 0) and in_aligned16
    NT = lds_nt(N)
    wg128 = cdiv(batch, 128) * cdiv(N, 32 * NT) * P
    return bool(S == 1 and lds_on and lds_ok and N >= LDS_MIN_N and batch >= LDS_MIN_ROWS and
                (batch <= LDS_MAXROWS or P >= LDS_MANY_P) and wg128 >= min_wg)


def lds_wide(N: int) -> bool:
    """k_dense_fwd_lds: the 16-byte store epilogue (N % 4 == 0; the output rows of the plan are then 16-byte aligned)."""
    return N % 4 == 0


def fwd_ring_variant(K, N, batch, P, w_off, in_aligned16) -> int:
    """pyz_gemm_ring.h pyz_fwd_ring_variant with PYZ_FWD_RING_WIDE unset (only so that a case can assert 0)."""
    n_cg = cdiv(N, 200) if N > 200 else 1
    wgs = cdiv(batch, 32) * P * n_cg
    if wgs < RING_MINWG or wgs > RING_MAXWG:
        return 0
    if K % 4 or N % 4 or w_off % 4 or not in_aligned16:
        return 0
    return 1 if RING_N[0] < N <= RING_N[1] else 0


# ---------------------------------------------------------------- cases
class DenseCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str
    P: int = 1
    batch: int = 70
    gathered: bool = False   # x has more rows than the batch; the batch comes through row_idx
    x_offset: bool = False   # x starts 4 bytes into its storage (no 16-byte aligned rows)
    env: dict = {}           # PYZ_FWD_LDS / PYZ_FWD_LDS_MINWG (both read per call)
    sgd: bool = False        # run sgd_step instead of loss_grad (k_wgrad_all<1> with its update epilogue)
    seed: int = 0            # added to the name's seed: picked so that relu layers keep their units alive

    @property
    def spec(self) -> o_mlp.MLPSpec:
        return o_mlp.MLPSpec(self.dims, self.acts, self.loss)

    @property
    def max_batch(self) -> int:
        """Rows of the plan: a few above the batch, so that the rows past it exist and must stay untouched."""
        return self.batch + 3


class Fwd(NamedTuple):
    layer: int
    kernel: str        # expression KernelProbe reports
    S: int
    exit: str          # why pyz_pick_waves stopped
    vec: int
    K: int
    N: int
    copy: bool         # writes the contiguous batch copy (layer 0 of a gathered fused gradient call)
    lds: Optional[tuple]   # (NT, wide) when k_dense_fwd_lds runs


class BwdData(NamedTuple):
    layer: int
    S: int
    exit: str
    vec: int
    K: int
    N: int
    act_prev: str


class Wgrad(NamedTuple):
    kernel: str        # expression KernelProbe reports
    S: int
    exit: str
    layers: tuple      # (K, N) of the layers the launch covers
    gather: str        # "", "copy" (reads the forward's batch copy) or "self" (gathers through row_idx)


class Launches(NamedTuple):
    fwd: list
    bwd_data: list
    wgrad: list


def wgrad_all_expr(S: int, plain: bool) -> str:
    """pyz_api.hip launch_wgrad_all: the kernel expression of each arm."""
    if S == 1:
        return "k_wgrad_all<1, true>" if plain else "k_wgrad_all<1>"   # (the probe reports it without the macro's parentheses)
    return f"k_wgrad_all<{S}>"


def expected_launches(case: DenseCase, batch: Optional[int] = None, call: str = "grad") -> Launches:
    """The Dense launches of `loss_grad` / `sgd_step` (call = "grad") or `forward` (call = "forward") for a case, in launch
    order per family.  Restates pyz_api.hip: launch_loss_backward (fused: hidden forwards, head, launch_bwd_data_hidden,
    launch_wgrad_all; else launch_forward, launch_loss, launch_backward) and pyz_mlp_forward (launch_forward over all layers)."""
    B = case.batch if batch is None else batch
    dims, P, D = case.dims, case.P, case.spec.n_params
    L = len(dims) - 1
    fused = can_fuse(dims)
    offs = w_offsets(dims)
    grad = call == "grad"
    copy0 = grad and fused and case.gathered and L > 1   # launch_loss_backward: xb = m->xb
    fwd = []
    for l in range(L - 1 if (grad and fused) else L):
        K, N = dims[l], dims[l + 1]
        aligned = not (l == 0 and case.x_offset)
        S, why = pick_waves(fwd_tiles(B, N) * P, fwd_steps(K))
        assert fwd_ring_variant(K, N, B, P, offs[l], aligned) == 0, f"{case.name}: layer {l} would take the ring kernel"
        lds = None
        kernel = "k_dense_fwd"
        if fwd_takes_lds(K, N, B, P, D, offs[l], S, aligned, int(case.env.get("PYZ_FWD_LDS", 1)),
                         int(case.env.get("PYZ_FWD_LDS_MINWG", LDS_MINWG))):
            lds = (lds_nt(N), lds_wide(N))
            kernel = f"k_dense_fwd_lds<{lds[0]}>"
        fwd.append(Fwd(l, kernel, S, why, fwd_vec(K, aligned), K, N, copy0 and l == 0, lds))
    if not grad:
        return Launches(fwd, [], [])
    bwd = []
    for l in range(L - 2 if fused else L - 1, 0, -1):   # the head kernel produces delta[L-2] of a fused model
        K, N = dims[l], dims[l + 1]
        S, why = pick_waves(bwd_data_tiles(B, K) * P, bwd_data_steps(N))
        bwd.append(BwdData(l, S, why, bwd_data_vec(N, offs[l], P, D), K, N, case.acts[l - 1]))
    layers = tuple(zip(dims[:-1], dims[1:]))
    if fused:
        tiles = sum(wgrad_tiles(K, N) for K, N in layers)
        S, why = pick_waves(tiles * P, wgrad_steps(B))
        gather = ("copy" if L > 1 else "self") if case.gathered else ""
        wg = [Wgrad(wgrad_all_expr(S, not case.sgd), S, why, layers, gather)]
    else:
        wg = []
        for l in range(L - 1, -1, -1):
            K, N = layers[l]
            S, why = pick_waves(wgrad_tiles(K, N) * P, wgrad_steps(B))
            wg.append(Wgrad("k_dense_bwd_weight", S, why, (layers[l],), "self" if (case.gathered and l == 0) else ""))
    return Launches(fwd, bwd, wg)


def _wave_ranges(steps: int, S: int):
    return [((steps * w) // S, (steps * (w + 1)) // S) for w in range(S)]


def _has_16_4_1(n: int) -> bool:
    """A wave's range of n steps leaves the 16-, 4- and 1-step groups of k_dense_bwd_weight all non-empty."""
    return n >= 16 and (n % 16) >= 4 and (n % 4) >= 1


# ---------------------------------------------------------------- the coverage table
SS = (1, 2, 4, 8, 16)
CELLS = frozenset(
    # k_dense_fwd
    [f"fwd S={S} vec={v}" for S in SS for v in (0, 1)] +
    [f"fwd S={S} exit={e}" for S in (2, 4, 8) for e in ("steps", "tiles")] +
    [f"fwd K={K}" for K in (28, 29, 60, 61, 124, 125, 252, 253)] +
    ["fwd K odd", "fwd fewer 8-chunks than waves"] +
    [f"fwd N={N}" for N in (31, 32, 33)] + ["fwd ragged column tile N>64"] +
    [f"fwd batch={b}" for b in (1, 31, 32, 33)] + ["fwd ragged row tile", "fwd x offset K%8==0", "fwd P>1 odd D"] +
    # batch copy of k_dense_fwd
    [f"copy tiles_n={t} {path}" for t in ("1", "2", ">=3") for path in ("vec S>1", "pair tail S>1")] +
    # rows_cap
    ["rows_cap forward", "rows_cap loss_grad"] +
    # k_dense_fwd_lds
    [f"lds NT={nt} {ep}" for nt in (2, 4, 7) for ep in ("16-byte", "dword")] +
    [f"lds K%16={r}" for r in (0, 4, 12)] +
    ["lds two column tiles ragged", "lds batch%128!=0", "lds gather copy", "lds no override"] +
    # k_dense_bwd_data
    [f"bwd_data S={S} vec={v}" for S in SS for v in (0, 1)] +
    ["bwd_data N odd", "bwd_data w_off%4!=0 N%8==0"] + [f"bwd_data K={K}" for K in (31, 32, 33)] +
    [f"bwd_data act={a} K>=33" for a in ("relu", "tanh", "sigmoid", "linear")] + ["bwd_data three hidden layers"] +
    # k_dense_bwd_weight
    [f"bwd_weight S={S} gather={g}" for S in SS for g in (0, 1)] +
    ["bwd_weight batch odd", "bwd_weight groups 16+4+1", "bwd_weight K+1=32", "bwd_weight K+1=33", "bwd_weight P>1"] +
    # k_wgrad_all
    ["wgrad_all <1, true>", "wgrad_all <1>"] + [f"wgrad_all <{S}> batch {par}" for S in (2, 4, 8, 16) for par in ("odd", "even")] +
    ["wgrad_all gather copy", "wgrad_all gather self", "wgrad_all K+1=32", "wgrad_all K+1=33", "wgrad_all three layers",
     "wgrad_all P>1"])


def reached_cells(case: DenseCase) -> set:
    """The cells of the table a case reaches, from `expected_launches` alone."""
    B, P, D = case.batch, case.P, case.spec.n_params
    la = expected_launches(case)
    cells = set()
    for f in la.fwd:
        if f.lds:
            NT, wide = f.lds
            cells.add(f"lds NT={NT} {'16-byte' if wide else 'dword'}")
            if f.K % 16 in (0, 4, 12):
                cells.add(f"lds K%16={f.K % 16}")
            if f.N > 224 and f.N % 224:
                cells.add("lds two column tiles ragged")
            if B % 128:
                cells.add("lds batch%128!=0")
            if f.copy:
                cells.add("lds gather copy")
            if not case.env:
                cells.add("lds no override")
            continue
        cells.add(f"fwd S={f.S} vec={f.vec}")
        if f.S in (2, 4, 8):
            cells.add(f"fwd S={f.S} exit={f.exit}")
        cells.add(f"fwd K={f.K}")
        if f.K % 2:
            cells.add("fwd K odd")
        if (f.K >> 3 if f.vec else 0) < f.S and f.S > 1:
            cells.add("fwd fewer 8-chunks than waves")
        cells.add(f"fwd N={f.N}")
        if f.N > 64 and f.N % 32:
            cells.add("fwd ragged column tile N>64")
        cells.add(f"fwd batch={B}")
        if B > 32 and B % 32:
            cells.add("fwd ragged row tile")
        if f.layer == 0 and case.x_offset and f.K % 8 == 0:
            cells.add("fwd x offset K%8==0")
        if P > 1 and D % 2:
            cells.add("fwd P>1 odd D")
        if f.copy and B % 32 and f.S > 1:
            tn = cdiv(f.N, 32)
            t = str(tn) if tn < 3 else ">=3"
            if f.vec:
                cells.add(f"copy tiles_n={t} vec S>1")
            elif f.K % 2:
                cells.add(f"copy tiles_n={t} pair tail S>1")
    if not case.gathered and not case.sgd:
        if any(not f.lds for f in expected_launches(case, call="forward").fwd):
            cells.add("rows_cap forward")
        if any(not f.lds and f.layer > 0 for f in la.fwd):   # (layer 0 of loss_grad carries the step scalars instead)
            cells.add("rows_cap loss_grad")
    offs = w_offsets(case.dims)
    for b in la.bwd_data:
        cells.add(f"bwd_data S={b.S} vec={b.vec}")
        if b.N % 2:
            cells.add("bwd_data N odd")
        if b.N % 8 == 0 and offs[b.layer] % 4:
            cells.add("bwd_data w_off%4!=0 N%8==0")
        cells.add(f"bwd_data K={b.K}")
        if b.K >= 33:
            cells.add(f"bwd_data act={b.act_prev} K>=33")
    if len(case.dims) - 2 >= 3 and la.bwd_data:
        cells.add("bwd_data three hidden layers")
    for wg in la.wgrad:
        if wg.kernel == "k_dense_bwd_weight":
            (K, N), = wg.layers
            cells.add(f"bwd_weight S={wg.S} gather={int(wg.gather == 'self')}")
            if B % 2:
                cells.add("bwd_weight batch odd")
            if any(_has_16_4_1(e - s) for s, e in _wave_ranges(wgrad_steps(B), wg.S)):
                cells.add("bwd_weight groups 16+4+1")
            if K + 1 in (32, 33):
                cells.add(f"bwd_weight K+1={K + 1}")
            if P > 1:
                cells.add("bwd_weight P>1")
        else:
            if wg.S == 1:
                cells.add("wgrad_all <1>" if case.sgd else "wgrad_all <1, true>")
            else:
                cells.add(f"wgrad_all <{wg.S}> batch {'odd' if B % 2 else 'even'}")
            if wg.gather:
                cells.add(f"wgrad_all gather {wg.gather}")
            for K, N in wg.layers:
                if K + 1 in (32, 33):
                    cells.add(f"wgrad_all K+1={K + 1}")
            if len(wg.layers) >= 3:
                cells.add("wgrad_all three layers")
            if P > 1:
                cells.add("wgrad_all P>1")
    return cells & CELLS


def _c(name, dims, acts, loss, P=1, batch=70, gathered=False, x_offset=False, env=None, sgd=False, seed=0):
    return DenseCase(name, tuple(dims), tuple(acts), loss, P, batch, gathered, x_offset, dict(env or {}), sgd, seed)


SC, MS = "scce", "mse"
LDS_ANY = {"PYZ_FWD_LDS_MINWG": "1"}     # take k_dense_fwd_lds whenever the shape allows it
LDS_OFF = {"PYZ_FWD_LDS": "0"}

R, T, G, LN, SM = "relu", "tanh", "sigmoid", "linear", "softmax"

CASES = [
    # ---- k_dense_fwd on layer 0 of a fused model (the head takes the last layer): every S at both sides of its K boundary,
    # float4 and pair path; column / row tile edges; the weight gradient as k_wgrad_all<S> by the batch
    _c("fwd_k24_s1_vec_n31_b1", (24, 31, 3), (T, SM), SC, batch=1),
    _c("fwd_k28_s1_n32_b31", (28, 32, 4), (R, SM), SC, batch=31),
    _c("fwd_k29_s2_odd_n33_b32", (29, 33, 5), (G, SM), SC, batch=32),
    _c("fwd_k32_s2_vec_b33", (32, 40, 10), (R, SM), SC, batch=33),
    _c("fwd_k60_s2_b62", (60, 40, 2), (T, LN), MS, batch=62),
    _c("fwd_k61_s4_odd_b63", (61, 40, 10), (R, SM), SC, batch=63),
    _c("fwd_k64_s4_vec_n70", (64, 70, 8), (G, G), MS, batch=70),
    _c("fwd_k64_s4_xoff", (64, 40, 10), (R, SM), SC, batch=45, x_offset=True),
    _c("fwd_k124_s4_b126", (124, 40, 10), (LN, SM), SC, batch=126),
    _c("fwd_k125_s8_odd_b127", (125, 40, 10), (R, SM), SC, batch=127),
    _c("fwd_k128_s8_vec_n100", (128, 100, 10), (T, SM), SC, batch=200),
    _c("fwd_k252_s8_b254", (252, 40, 6), (R, T), MS, batch=254),
    _c("fwd_k253_s16_odd_b255", (253, 40, 10), (G, SM), SC, batch=255),
    _c("fwd_k256_s16_vec_b256", (256, 40, 10), (R, SM), SC, batch=256),
    _c("fwd_k256_s16_xoff", (256, 33, 10), (T, SM), SC, batch=70, x_offset=True),
    _c("fwd_p3_odd_d", (28, 33, 5), (R, SM), SC, P=3, batch=70),
    _c("fwd_p3_odd_d_k61", (61, 32, 4), (T, SM), SC, P=3, batch=45, gathered=True),
    # ---- the S loop of pyz_pick_waves ending on the tile count (tiles x S reached the target), several particles
    _c("fwd_tiles_s2_p32", (64, 512, 10), (R, SM), SC, P=32, batch=70),
    _c("fwd_tiles_s4_p16", (128, 512, 10), (T, SM), SC, P=16, batch=70, gathered=True),
    _c("fwd_tiles_s8_p8", (256, 512, 10), (R, SM), SC, P=8, batch=70),
    # ---- the batch copy: layer 0 of a gathered fused gradient, 1 / 2 / 3+ column tiles, ragged batch, S > 1
    _c("copy_t1_vec", (64, 31, 10), (R, SM), SC, batch=70, gathered=True),
    _c("copy_t2_vec", (128, 40, 10), (T, SM), SC, batch=45, gathered=True),
    _c("copy_t3_vec", (64, 70, 10), (R, SM), SC, batch=131, gathered=True),
    _c("copy_t5_vec_s16", (256, 150, 10), (G, SM), SC, batch=77, gathered=True),
    _c("copy_t1_pair", (61, 32, 3), (T, LN), MS, batch=70, gathered=True),
    _c("copy_t2_pair", (125, 33, 10), (R, SM), SC, batch=61, gathered=True),
    _c("copy_t4_pair", (61, 100, 10), (R, SM), SC, batch=99, gathered=True),
    _c("copy_t3_pair_s16", (253, 90, 10), (LN, SM), SC, batch=35, gathered=True),
    # ---- k_dense_fwd_lds: NT x epilogue, slab remainders, two column tiles, ragged rows, gather with copy
    _c("lds_nt2_wide_k16", (16, 64, 10), (R, SM), SC, batch=130, env=LDS_ANY),
    _c("lds_nt2_dword_k20", (20, 50, 10), (T, SM), SC, batch=128, env=LDS_ANY),
    _c("lds_nt4_wide_k28_copy", (28, 128, 10), (R, SM), SC, batch=200, gathered=True, env=LDS_ANY),
    _c("lds_nt4_dword_k16", (16, 126, 4), (G, LN), MS, P=2, batch=150, env=LDS_ANY),
    _c("lds_nt7_wide_two_tiles", (28, 252, 10), (R, SM), SC, batch=140, env=LDS_ANY),
    _c("lds_nt7_dword_two_tiles", (20, 250, 10), (T, SM), SC, P=2, batch=129, gathered=True, env=LDS_ANY),
    _c("lds_nt7_one_tile_off", (24, 224, 10), (R, SM), SC, batch=140, env=LDS_OFF),
    _c("lds_default_p64", (36, 96, 96, 10), (R, T, SM), SC, P=64, batch=500, gathered=True),
    # ---- k_dense_bwd_data: fused models with two or three hidden layers (layers L-2 .. 1)
    _c("bwdd_n16_s1_vec", (11, 33, 16, 4), (R, T, SM), SC, batch=70),
    _c("bwdd_n15_s1", (12, 31, 15, 4), (T, R, SM), SC, batch=33),
    _c("bwdd_n31_s2_k32", (12, 32, 31, 10), (G, R, SM), SC, batch=70, gathered=True),
    _c("bwdd_n32_s2_vec", (11, 40, 32, 10), (T, G, SM), SC, batch=62),
    _c("bwdd_n32_woff", (12, 33, 32, 10), (LN, R, SM), SC, batch=70),
    _c("bwdd_n63_s4", (12, 40, 63, 10), (G, T, SM), SC, batch=100),
    _c("bwdd_n64_s4_vec", (15, 48, 64, 3), (R, LN, LN), MS, batch=70),
    _c("bwdd_n127_s8", (12, 36, 127, 10), (LN, R, SM), SC, batch=50),
    _c("bwdd_n128_s8_vec_p2", (15, 40, 128, 12), (T, R, SM), SC, P=2, batch=70),
    _c("bwdd_n255_s16", (12, 33, 255, 10), (R, T, SM), SC, batch=40),
    _c("bwdd_n256_s16_vec", (11, 64, 256, 10), (G, R, SM), SC, batch=70),
    _c("bwdd_three_hidden", (31, 40, 64, 33, 10), (T, G, R, SM), SC, batch=96, gathered=True),
    # ---- unfused models (last layer wider than 32): k_dense_fwd on every layer, k_dense_bwd_data down to layer 1,
    # k_dense_bwd_weight per layer with S by the batch, gathered at layer 0
    _c("unf_b16_s1", (31, 40, 33), (R, SM), SC, batch=16, gathered=True),
    _c("unf_b31_s2", (32, 33, 40), (T, LN), MS, batch=31, gathered=True),
    _c("unf_b63_s4", (12, 40, 48), (G, SM), SC, batch=63, gathered=True),
    _c("unf_b127_s8_p2", (20, 32, 36), (R, T), MS, P=2, batch=127, gathered=True),
    _c("unf_b255_s16", (12, 31, 40), (T, SM), SC, batch=255, gathered=True),
    _c("unf_b701_groups", (31, 24, 40), (R, SM), SC, batch=701, gathered=True),
    _c("unf_b700_plain", (32, 20, 36), (LN, G), MS, batch=700),
    _c("unf_n256_bwdd_s16", (12, 40, 256), (R, SM), SC, batch=70),
    _c("unf_n255_three_hidden", (12, 33, 40, 34, 255), (T, R, G, LN), MS, batch=45),
    # ---- k_wgrad_all: the update epilogue, one layer gathering for itself, odd / even batches per S, three layers
    _c("wg_sgd_s1", (20, 16, 4), (R, SM), SC, batch=30, sgd=True),
    _c("wg_l1_self_gather", (31, 10), (SM,), SC, batch=63, gathered=True),
    _c("wg_l1_self_gather_p2", (32, 5), (LN,), MS, P=2, batch=256, gathered=True),
    _c("wg_s2_odd", (31, 20, 10), (R, SM), SC, batch=61),
    _c("wg_s4_even", (32, 24, 10), (T, SM), SC, batch=64, gathered=True),
    _c("wg_s8_even_l3", (16, 31, 32, 10), (R, R, SM), SC, batch=128),
    _c("wg_s16_odd_l3_p2", (20, 32, 31, 6), (G, T, LN), MS, P=2, batch=301, gathered=True),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"

# ---------------------------------------------------------------- data
EDGE = 8.0   # weight of the last reduction index of every kernel against the rest


def case_data(case: DenseCase):
    """Seeded inputs of a case: (x rows, labels / targets, row_idx or None, thetas (P, D)), float32 / int32, drawn as
    head_cases.case_data draws them, with the edges weighted: the last input column, the last batch row and the last row
    of every W (the last reduction index of the forward pass, of the weight gradients, and -- through the delta it
    scales -- of the data gradient) carry EDGE times the rest, so a kernel that drops or doubles an edge element misses
    by far more than the bound.  Every layer is then scaled so that its float64 pre-activations over the other batch rows
    have unit rms: tanh and sigmoid stay out of saturation."""
    spec, B = case.spec, case.batch
    rng = np.random.default_rng(sum(map(ord, case.name)) + 100003 * case.seed)
    n_rows = B + B // 5 + 3 if case.gathered else B
    x = rng.normal(size=(n_rows, spec.dims[0])).astype(np.float32)
    N = spec.dims[-1]
    if case.loss == "scce":
        y = rng.integers(0, N, size=n_rows).astype(np.int32)
    elif spec.acts[-1] == "sigmoid":
        y = rng.uniform(0.0, 1.0, size=(n_rows, N)).astype(np.float32)
    elif spec.acts[-1] == "tanh":
        y = rng.uniform(-1.0, 1.0, size=(n_rows, N)).astype(np.float32)
    else:
        y = rng.normal(size=(n_rows, N)).astype(np.float32)
    idx = rng.permutation(n_rows)[:B].astype(np.int32) if case.gathered else None
    heavy = int(idx[B - 1]) if case.gathered else B - 1
    x[:, -1] *= EDGE
    x[heavy] *= EDGE
    rows = (x if idx is None else x[idx]).astype(np.float64)
    light = rows[:-1] if B > 1 else rows
    thetas = np.empty((case.P, spec.n_params), dtype=np.float32)
    for p in range(case.P):
        parts, h = [], light
        for (fan_in, fan_out), act in zip(zip(spec.dims[:-1], spec.dims[1:]), spec.acts):
            w = rng.normal(size=(fan_in, fan_out))
            b = rng.normal(size=fan_out) * 0.2
            w[-1] *= EDGE
            z = h @ w + b
            s = 1.0 / np.sqrt(np.mean(z * z))
            parts += [(w * s).reshape(-1), b * s]
            h = o_mlp._act(z * s, act)
        thetas[p] = np.concatenate(parts).astype(np.float32)
    return x, y, idx, thetas


def batch_rows(case: DenseCase, x, y, idx, batch: Optional[int] = None):
    """The rows and targets the first `batch` batch rows use."""
    B = case.batch if batch is None else batch
    return (x[:B], y[:B]) if idx is None else (x[idx[:B]], y[idx[:B]])


def reference_stats(case: DenseCase):
    """Per layer of the float64 reference, worst particle: (share of pre-activations within +-4, share of units whose
    output is zero over the whole batch)."""
    x, y, idx, thetas = case_data(case)
    rows, _ = batch_rows(case, x, y, idx)
    spec = case.spec
    within, dead = [1.0] * spec.n_layers, [0.0] * spec.n_layers
    for p in check_particles(case.P):
        h = rows.astype(np.float64)
        for l, ((w, b), act) in enumerate(zip(o_mlp.unpack(thetas[p].astype(np.float64), spec), spec.acts)):
            z = h @ w + b
            h = o_mlp._act(z, act)
            within[l] = min(within[l], float(np.mean(np.abs(z) <= 4.0)))
            dead[l] = max(dead[l], float(np.mean(np.all(h == 0.0, axis=0))))
    return within, dead


def check_particles(P: int):
    """The particles a case compares with the oracle: the first, the middle and the last."""
    return sorted({0, P // 2, P - 1})
