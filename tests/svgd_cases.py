"""The case table of the SVGD sweeps and the comparisons both SVGD matrix tests share (a plain module).

pyz_svgd_step runs its second phase on one of many arms (pyz_api.hip: svgd_sweep_impl, svgd_kernel_matrix_impl,
svgd_launch_distance_pass, svgd_gram_groups_impl): the Gauss-Seidel sweep as one resident launch (two kernels), one launch
per particle, or two per-row kernels per particle; the Jacobi sweep on the all-rows-at-once kernels (distances through the
Gram matrix on the float64 matrix cores in three instantiations, or pairwise; fixed or median bandwidth) or on the per-row
kernels.  This module restates which kernels a case launches (`expected_svgd_launches`, `expected_group_launches`), names
the cells of the coverage table (`CELLS`, `reached_cells`), lists cases that reach every cell, builds their data (three
kinds: repulsion only, drive only, coupled), restates one sweep on top of oracle.svgd in a chosen dtype with the wrong
variants the sensitivity check needs (`ref_sweep`, `MUTATIONS`), and holds the comparisons: squared distances
(`compare_distances`), phi element by element as Adam's first step from a zero state leaves it (`compare_phi`), one Adam
step from a non-zero state (`compare_adam`) and the step's loss.  tests/test_svgd_dispatch_table.py pins all of it to the
source and to oracle.svgd on the CPU; tests/test_gpu_svgd_matrix.py runs the cases on the device."""

from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import numpy as np

from dense_cases import can_fuse
from oracle import mlp as o_mlp
from oracle import svgd as o_svgd

# ---------------------------------------------------------------- the rules (csrc/pyz_kernels.h, pyz_api.hip)
CUS = 256                 # compute units of the MI355X (pyz_cu_count)
GS_RANGE = 256 * 3        # elements of D per workgroup of k_svgd_gs and the resident kernels (256 * PYZ_GS_E)
GS_MAX_D = 256 * GS_RANGE  # 196 608: beyond it the Gauss-Seidel sweep runs the per-row kernels
ROW_BLOCK = 4 * 2 * 256   # PYZ_SVGD_BLOCK_ELEMS: elements of D per workgroup of k_svgd_dist
SV_E = 128                # PYZ_SV_E: elements staged per pass of the tile kernels
GROUPS = 8                # PYZ_SVGD_GROUPS
TILE_MAX_M = 64
ENV_DEFAULTS = {"PYZ_SVGD_TILES": 1, "PYZ_SVGD_GRAM": 1, "PYZ_SVGD_GS_FUSED": 1, "PYZ_SVGD_GS_RESIDENT": 1, "PYZ_SVGD_GS_ZIGZAG": 1}
ENV_NEVER = "PYZ_SVGD_GS_SPIN_LIMIT"     # no case sets it
C1 = float(np.float32(1.0) - np.float32(0.9))       # the kernels' (1.0f - 0.9f), not float32(0.1)
C2 = float(np.float32(1.0) - np.float32(0.999))
LR = 0.01
BLOCK_FLOOR, ELEM_FLOOR = 0.04, 0.25     # of the coupled cases' spread: see _svgd_data
T_ADAM = 7                # the Adam step of observable (c)


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def tile_range(D: int) -> int:
    """svgd_tile_layout: elements of D per workgroup of the distance pass, one round of workgroups on 256 CUs."""
    return SV_E * cdiv(D, 256 * SV_E)


def tile_blocks(D: int) -> int:
    return cdiv(D, tile_range(D))


class SvgdCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str
    M: int
    batch: int
    sweep: str               # "gs" or "jacobi"
    kind: str                # "rep" (repulsion only), "drive" (K = I) or "coupled"
    gamma: object = 0.37     # the bandwidth (passed as a float32), or "median"
    row0: int = 0
    n_local: Optional[int] = None
    env: tuple = ()          # ((switch, value), ...) set per call
    snap_off: bool = False   # the snapshot as a view 4 bytes off 16-byte alignment
    twin: bool = False       # particles 0 and 1 identical
    big: bool = False        # one step only, no wrong variants (the two large models)
    seed: int = 0

    @property
    def spec(self) -> o_mlp.MLPSpec:
        return o_mlp.MLPSpec(self.dims, self.acts, self.loss)

    @property
    def D(self) -> int:
        return self.spec.n_params

    @property
    def nl(self) -> int:
        return self.M if self.n_local is None else self.n_local

    @property
    def median(self) -> bool:
        return self.gamma == "median"

    @property
    def shard(self) -> bool:
        return self.nl != self.M

    @property
    def fused_head(self) -> bool:
        return can_fuse(self.dims)

    @property
    def g32(self) -> float:
        """The bandwidth as the library receives it: a float32 (0.37 is not one; the arithmetic runs on this input)."""
        return float(np.float32(self.gamma))

    @property
    def dist_form(self) -> str:
        """"gram" where the squared distances come from the Gram matrix (the Jacobi tile kernels by default), else "pairwise"."""
        return "gram" if self.sweep == "jacobi" and jacobi_arm(self) == "tile" and self.flag("PYZ_SVGD_GRAM") else "pairwise"

    def flag(self, name: str) -> int:
        return int(dict(self.env).get(name, ENV_DEFAULTS[name]))


def tile_shape(n_local: int, n_total: int, row0: int) -> bool:
    """svgd_tile_shape (the snapshot is never the written buffer: svgd_check_snapshot refuses that)."""
    return n_total <= TILE_MAX_M and row0 % 4 == 0 and n_local % 4 == 0


def distance_kernel(row0: int, n_rows: int, gram: bool) -> str:
    """svgd_launch_distance_pass."""
    if not gram:
        return "k_svgd_dist_tile"
    rb_lo, rb_hi = row0 >> 4, (row0 + n_rows - 1) >> 4
    if rb_hi == rb_lo:
        return "k_svgd_gram_tile<1,false>"
    if rb_hi == rb_lo + 1:
        return "k_svgd_gram_tile<2,false>"
    return "k_svgd_gram_tile<4,true>"


def gs_arm(case: SvgdCase, cu_count: int = CUS) -> str:
    """The arm of the Gauss-Seidel sweep: "resident", "resident2", "launch" (k_svgd_gs) or "rows"."""
    if not (case.flag("PYZ_SVGD_GS_FUSED") and case.M <= TILE_MAX_M and case.D <= GS_MAX_D):
        return "rows"
    mode = case.flag("PYZ_SVGD_GS_RESIDENT")
    reducers = cdiv(case.M, 8) if mode == 2 else cdiv(case.M, 4)
    if mode != 0 and cdiv(case.D, GS_RANGE) + reducers <= cu_count:
        return "resident2" if mode == 2 else "resident"
    return "launch"


def jacobi_arm(case: SvgdCase) -> str:
    """"tile" (kernel matrix + combine) or "rows"."""
    ok = tile_shape(case.nl, case.M, case.row0)
    return "tile" if ok and (case.flag("PYZ_SVGD_TILES") or case.median) else "rows"


def expected_svgd_launches(case: SvgdCase, cu_count: int = CUS) -> tuple:
    """The kernel expressions KernelProbe reports behind the gradient pass of pyz_svgd_step, in launch order (spaces and
    the macro's parentheses removed): k_loss_finalize of an unfused head, then svgd_sweep_impl."""
    out = [] if case.fused_head else ["k_loss_finalize"]
    if case.sweep == "jacobi":
        if jacobi_arm(case) == "tile":
            rows = (0, case.M) if case.median else (case.row0, case.nl)      # svgd_tile_layout: dist_row0, dist_rows
            out.append(distance_kernel(rows[0], rows[1], bool(case.flag("PYZ_SVGD_GRAM"))))
            if case.median:
                out += ["k_svgd_kmat", "k_svgd_median"]
            out += ["k_svgd_kmat", "k_svgd_update_tile"]                     # (the loss rides in k_svgd_update_tile)
            return tuple(out)
        assert not case.median, "the median bandwidth needs the tile shape"
        return tuple(out + ["k_svgd_dist", "k_svgd_update", "k_svgd_loss"])
    arm = gs_arm(case, cu_count)
    if arm in ("resident", "resident2"):
        return tuple(out + ["k_svgd_gs_resident2" if arm == "resident2" else "k_svgd_gs_resident", "k_svgd_loss"])
    if arm == "launch":
        zig = case.flag("PYZ_SVGD_GS_ZIGZAG")
        out += ["k_svgd_gs<true>" if zig and (i & 1) == 0 else "k_svgd_gs<false>" for i in range(-1, case.M)]
    else:
        out += ["k_svgd_dist", "k_svgd_update"] * case.M
    return tuple(out + ["k_svgd_loss"])


def expected_group_launches(M: int, D: int, g_lo: int, g_hi: int, gram: bool) -> tuple:
    """svgd_gram_groups_impl: the distance pass over the groups' blocks (none when they hold no block), all rows, then
    k_svgd_group_reduce."""
    nblk = tile_blocks(D)
    nb8 = cdiv(nblk, GROUPS)
    blk0, blk1 = min(g_lo * nb8, nblk), min(g_hi * nb8, nblk)
    return ((distance_kernel(0, M, gram),) if blk1 > blk0 else ()) + ("k_svgd_group_reduce",)


def svgd_kernels(launches) -> tuple:
    """KernelProbe's launches down to what `expected_svgd_launches` lists."""
    names = [n.replace(" ", "").strip("()") for n, _ in launches]
    return tuple(n for n in names if n.startswith("k_svgd") or n == "k_loss_finalize")


# ---------------------------------------------------------------- the coverage table
CELLS = frozenset([
    "gs k_svgd_gs_resident", "gs k_svgd_gs_resident2", "gs k_svgd_gs<true/false> alternating", "gs k_svgd_gs<false> only",
    "gs per-row by switch", "gs per-row because M > 64", "gs per-row because D > 196608",
    "gs per-launch chosen by the residency gate", "gs resident2 where mode 1 does not fit",
    "jacobi k_svgd_gram_tile<1,false> shard", "jacobi k_svgd_gram_tile<2,false> shard",
    "jacobi k_svgd_gram_tile<4,true> whole matrix", "jacobi k_svgd_gram_tile<1,false> whole matrix in one row block",
    "jacobi k_svgd_gram_tile<4,true> non-whole range over three row blocks",
    "jacobi k_svgd_dist_tile whole matrix (mirrored blocks)", "jacobi k_svgd_dist_tile rectangular shard",
    "median M=12 (144 values padded to 256)", "median M=8 (64 values, no padding)", "median M=64 (4096 values)",
    "median on a shard (distances of all rows)",
    "jacobi per-row by switch", "jacobi per-row because M % 4 != 0", "jacobi per-row because row0 % 4 != 0",
    "jacobi per-row because M > 64",
    "Gram fetch D odd", "Gram fetch D even",
    "D < 128", "D < 768", "ragged last 768-block, last wave partly out", "D % 128 != 0",
    "M < 64 with the j >= M padding live (M = 5)", "M < 64 with the j >= M padding live (M = 12)", "M = 1",
    "two identical particles", "snapshot 4 bytes off 16-byte alignment: k_svgd_dist",
    "snapshot 4 bytes off 16-byte alignment: k_svgd_dist_tile",
    "loss of a fused head", "loss of an unfused head (k_loss_finalize)", "loss of a shard (divided by M)",
    "kind rep", "kind drive", "kind coupled", "gamma 0.37", "gamma 2.5", "gamma median",
    "(c) Adam from a non-zero state: gs", "(c) Adam from a non-zero state: jacobi",
] + [f"k_svgd_dist D%4={r}" for r in range(4)] + [f"k_svgd_dist_tile D%4={r}" for r in range(4)])
GROUP_CELLS = frozenset(["groups: block count below 8", "groups: block count no multiple of 8",
                         "groups: 32 blocks per group (the most the layout gives)", "groups: a range that holds no block",
                         "groups: Gram D odd", "groups: Gram D even", "groups: two identical particles"])


def reached_cells(case: SvgdCase, cu_count: int = CUS) -> set:
    """The cells a case reaches, from its shape and `expected_svgd_launches` alone."""
    la, D, M = expected_svgd_launches(case, cu_count), case.D, case.M
    cells = {f"kind {case.kind}", "gamma median" if case.median else f"gamma {case.gamma}",
             "loss of a fused head" if case.fused_head else "loss of an unfused head (k_loss_finalize)"}
    if case.shard:
        cells.add("loss of a shard (divided by M)")
    if case.sweep == "gs":
        arm = gs_arm(case, cu_count)
        if arm == "resident":
            cells.add("gs k_svgd_gs_resident")
        elif arm == "resident2":
            cells.add("gs k_svgd_gs_resident2")
            if gs_arm(case._replace(env=()), cu_count) == "launch":
                cells.add("gs resident2 where mode 1 does not fit")
        elif arm == "launch":
            cells.add("gs k_svgd_gs<true/false> alternating" if "k_svgd_gs<true>" in la else "gs k_svgd_gs<false> only")
            if case.flag("PYZ_SVGD_GS_RESIDENT") != 0:
                cells.add("gs per-launch chosen by the residency gate")
        elif not case.flag("PYZ_SVGD_GS_FUSED"):
            cells.add("gs per-row by switch")
        elif M > TILE_MAX_M:
            cells.add("gs per-row because M > 64")
        else:
            assert D > GS_MAX_D
            cells.add("gs per-row because D > 196608")
        if arm != "rows":
            if D < GS_RANGE:
                cells.add("D < 768")
            if D % GS_RANGE and (D % GS_RANGE) % 192:
                cells.add("ragged last 768-block, last wave partly out")
    else:
        if jacobi_arm(case) == "tile":
            k, whole = la[0 if case.fused_head else 1], not case.shard
            if k == "k_svgd_dist_tile":
                cells.add("jacobi k_svgd_dist_tile whole matrix (mirrored blocks)" if whole or case.median
                          else "jacobi k_svgd_dist_tile rectangular shard")
                cells.add(f"k_svgd_dist_tile D%4={D % 4}")
                if case.snap_off and D % 4 == 0:
                    cells.add("snapshot 4 bytes off 16-byte alignment: k_svgd_dist_tile")
            else:
                cells.add("Gram fetch D odd" if D % 2 else "Gram fetch D even")
                n = k[len("k_svgd_gram_tile<")]
                if n == "4":
                    cells.add("jacobi k_svgd_gram_tile<4,true> whole matrix" if whole or case.median
                              else "jacobi k_svgd_gram_tile<4,true> non-whole range over three row blocks")
                elif whole or case.median:
                    assert n == "1"
                    cells.add("jacobi k_svgd_gram_tile<1,false> whole matrix in one row block")
                else:
                    cells.add(f"jacobi k_svgd_gram_tile<{n},false> shard")
            if case.median:
                cells.add({12: "median M=12 (144 values padded to 256)", 8: "median M=8 (64 values, no padding)",
                           64: "median M=64 (4096 values)"}.get(M, ""))
                if case.shard:
                    cells.add("median on a shard (distances of all rows)")
            if D < SV_E:
                cells.add("D < 128")
            if D % SV_E:
                cells.add("D % 128 != 0")
        elif not case.flag("PYZ_SVGD_TILES") and tile_shape(case.nl, M, case.row0):
            cells.add("jacobi per-row by switch")
        elif M > TILE_MAX_M:
            cells.add("jacobi per-row because M > 64")
        elif case.row0 % 4:
            cells.add("jacobi per-row because row0 % 4 != 0")
        else:
            assert M % 4 or case.nl % 4
            cells.add("jacobi per-row because M % 4 != 0")
    if "k_svgd_dist" in la:
        cells.add(f"k_svgd_dist D%4={D % 4}")
        if case.snap_off and D % 4 == 0:
            cells.add("snapshot 4 bytes off 16-byte alignment: k_svgd_dist")
    if M in (5, 12) and "rows" not in (gs_arm(case, cu_count) if case.sweep == "gs" else jacobi_arm(case)):
        cells.add(f"M < 64 with the j >= M padding live (M = {M})")
    if M == 1:
        cells.add("M = 1")
    if case.twin:
        cells.add("two identical particles")
    if has_adam_step(case):
        cells.add(f"(c) Adam from a non-zero state: {case.sweep}")
    return cells & CELLS


def has_adam_step(case: SvgdCase) -> bool:
    """Observable (c) runs on the coupled cases (the large models run one step)."""
    return case.kind == "coupled" and not case.big


R, T, G, LN, SM = "relu", "tanh", "sigmoid", "linear", "softmax"
A = ((20, 16, 4), (R, SM), "scce")             # D = 404
A1 = ((20, 17, 4), (R, SM), "scce")            # D = 429 (the input width moves D by 16: the hidden width gives the residues)
A2 = ((20, 18, 4), (R, SM), "scce")            # D = 454
A3 = ((20, 15, 4), (R, SM), "scce")            # D = 379
B = ((6, 12, 8, 3), (T, G, LN), "mse")         # D = 215
W = ((64, 40, 24, 10), (R, R, SM), "scce")     # D = 3 834: five Gauss-Seidel blocks
WM = ((64, 40, 24, 10), (T, T, LN), "mse")
U = ((12, 20, 40), (T, SM), "scce")            # D = 1 100: unfused head
TINY = ((5, 7, 3), (T, SM), "scce")            # D = 66
BIG1 = ((784, 251, 10), (T, LN), "mse")        # D = 199 555 > 196 608
BIG2 = ((784, 240, 10), (T, LN), "mse")        # D = 190 810: 249 Gauss-Seidel blocks


def _c(name, model, M, batch, sweep, kind, gamma=0.37, **kw):
    env = tuple(sorted((k, int(v)) for k, v in kw.pop("env", {}).items()))
    return SvgdCase(name, tuple(model[0]), tuple(model[1]), model[2], M, batch, sweep, kind, gamma, env=env, **kw)


RES0, RES2 = {"PYZ_SVGD_GS_RESIDENT": 0}, {"PYZ_SVGD_GS_RESIDENT": 2}
PAIR = {"PYZ_SVGD_GRAM": 0}
CASES = [
    # ---- Gauss-Seidel: the two resident kernels, one launch per particle (alternating or ascending), the per-row kernels
    _c("gs_res_w_m7", W, 7, 9, "gs", "coupled"),
    _c("gs_res_b_m5_rep", B, 5, 11, "gs", "rep", 2.5),
    _c("gs_res_tiny_m5", TINY, 5, 7, "gs", "coupled", 2.5),
    _c("gs_res_a_m1", A, 1, 14, "gs", "drive"),
    _c("gs_res_a_m3_drive", A, 3, 13, "gs", "drive", 2.5),
    _c("gs_res_a1_m6_twin", A1, 6, 10, "gs", "coupled", twin=True),
    _c("gs_res_u_m6_unfused", U, 6, 23, "gs", "coupled", 2.5),
    _c("gs_res2_w_m12", W, 12, 8, "gs", "coupled", 2.5, env=RES2),
    _c("gs_res2_wm_m64_rep", WM, 64, 5, "gs", "rep", 2.5, env=RES2),
    _c("gs_zig_w_m9", W, 9, 9, "gs", "coupled", 2.5, env=RES0),
    _c("gs_zig_b_m5_rep", B, 5, 4, "gs", "rep", env=RES0),
    _c("gs_asc_a_m6", A, 6, 15, "gs", "coupled", env={"PYZ_SVGD_GS_RESIDENT": 0, "PYZ_SVGD_GS_ZIGZAG": 0}),
    _c("gs_rows_a3_m5", A3, 5, 12, "gs", "coupled", env={"PYZ_SVGD_GS_FUSED": 0}),
    _c("gs_rows_a1_m4", A1, 4, 6, "gs", "coupled", 2.5, env={"PYZ_SVGD_GS_FUSED": 0}),
    _c("gs_rows_a2_m3", A2, 3, 17, "gs", "coupled", 2.5, env={"PYZ_SVGD_GS_FUSED": 0}),
    _c("gs_rows_a_m65", A, 65, 5, "gs", "coupled", 2.5),
    _c("gs_rows_big_m3_rep", BIG1, 3, 4, "gs", "rep", 2.5, big=True),
    _c("gs_gate_big_m32_rep", BIG2, 32, 4, "gs", "rep", big=True),
    _c("gs_gate_big_m32_rep_res2", BIG2, 32, 4, "gs", "rep", big=True, env=RES2),
    # ---- Jacobi on the all-rows-at-once kernels: the three Gram instantiations, the pairwise kernel, the median bandwidth
    _c("j_gram1_w_shard", W, 24, 7, "jacobi", "coupled", row0=16, n_local=8),
    _c("j_gram2_b_shard_rep", B, 24, 6, "jacobi", "rep", 2.5, row0=12, n_local=8),
    _c("j_gram4_wm_m64_rep", WM, 64, 4, "jacobi", "rep"),
    _c("j_gram1_a_m12", A, 12, 14, "jacobi", "coupled", 2.5),
    _c("j_gram4_w_span3", W, 64, 6, "jacobi", "coupled", row0=8, n_local=40),
    _c("j_gram_tiny_m4", TINY, 4, 9, "jacobi", "coupled"),
    _c("j_gram_a_m8_twin", A, 8, 10, "jacobi", "coupled", 2.5, twin=True),
    _c("j_gram_a_m4_drive", A, 4, 12, "jacobi", "drive", 2.5),
    _c("j_gram_u_shard_unfused", U, 8, 19, "jacobi", "coupled", row0=4, n_local=4),
    _c("j_pair_a_m8", A, 8, 13, "jacobi", "coupled", env=PAIR),
    _c("j_pair_b_shard_rep", B, 12, 8, "jacobi", "rep", row0=4, n_local=8, env=PAIR),
    _c("j_pair_a1_m4", A1, 4, 5, "jacobi", "coupled", 2.5, env=PAIR),
    _c("j_pair_a2_shard", A2, 8, 16, "jacobi", "coupled", row0=4, n_local=4, env=PAIR),
    _c("j_pair_a_m8_off", A, 8, 11, "jacobi", "coupled", 2.5, env=PAIR, snap_off=True),
    _c("j_med_a_m12", A, 12, 14, "jacobi", "coupled", "median"),
    _c("j_med_a_m8_pair_shard", A, 8, 9, "jacobi", "coupled", "median", row0=4, n_local=4, env=PAIR),
    _c("j_med_b_m64_rep", B, 64, 4, "jacobi", "rep", "median"),
    # ---- Jacobi on the per-row kernels
    _c("j_rows_a_m8_switch", A, 8, 14, "jacobi", "coupled", 2.5, env={"PYZ_SVGD_TILES": 0}),
    _c("j_rows_a_m4_off", A, 4, 7, "jacobi", "coupled", 2.5, env={"PYZ_SVGD_TILES": 0}, snap_off=True),
    _c("j_rows_a1_m5", A1, 5, 10, "jacobi", "coupled", 2.5),
    _c("j_rows_a2_row0_2", A2, 8, 12, "jacobi", "coupled", 2.5, row0=2, n_local=3),
    _c("j_rows_b_m65_rep", B, 65, 4, "jacobi", "rep"),
    _c("j_rows_a3_m7_drive", A3, 7, 8, "jacobi", "drive", 2.5, row0=3, n_local=4),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"

# observable (a): (case whose model and particles are used, what it is there for)
DIST_CASES = ["j_gram2_b_shard_rep", "j_gram4_w_span3", "j_gram_u_shard_unfused", "j_gram_a_m8_twin", "gs_gate_big_m32_rep",
              "j_gram_tiny_m4"]


def group_cells(case: SvgdCase) -> set:
    nblk = tile_blocks(case.D)
    nb8 = cdiv(nblk, GROUPS)
    cells = {"groups: Gram D odd" if case.D % 2 else "groups: Gram D even"}
    if nblk < GROUPS:
        cells.add("groups: block count below 8")
    elif nblk % GROUPS:
        cells.add("groups: block count no multiple of 8")
    if nb8 == 32:
        cells.add("groups: 32 blocks per group (the most the layout gives)")
    if min(3 * nb8, nblk) == nblk or min(3 * nb8, nblk) == 0:
        cells.add("groups: a range that holds no block")
    if case.twin:
        cells.add("groups: two identical particles")
    return cells


# ---------------------------------------------------------------- data
class SvgdData(NamedTuple):
    x: np.ndarray            # (batch, in) float32
    y: np.ndarray
    parts: np.ndarray        # (M, D) float32: the whole particle matrix
    m0: np.ndarray           # (n_local, D) float32: Adam state of observable (c), the scale of phi with random signs
    v0: np.ndarray           # 0.25 .. 4 times the block scale of phi^2


def blocks(spec):
    for l, ((ko, bo), K, N) in enumerate(zip(spec.offsets(), spec.dims[:-1], spec.dims[1:])):
        yield f"W{l}", slice(ko, ko + K * N)
        yield f"b{l}", slice(bo, bo + N)


def last_layer(spec) -> slice:
    ko, bo = spec.offsets()[-1]
    return slice(ko, bo + spec.dims[-1])


@functools.lru_cache(maxsize=None)
def _svgd_data(case: SvgdCase) -> SvgdData:
    spec, M, D = case.spec, case.M, case.D
    rng = np.random.default_rng(sum(map(ord, case.name)) + 7919 * (case.seed + 1))
    x = rng.normal(size=(case.batch, spec.dims[0])).astype(np.float32)
    if spec.dims[0] > 100:
        x *= np.float32(0.2)             # (tanh of the large models stays out of saturation)
    if case.loss == "scce":
        y = rng.integers(0, spec.dims[-1], size=case.batch).astype(np.int32)
    elif case.kind == "rep":
        y = np.zeros((case.batch, spec.dims[-1]), dtype=np.float32)
    else:
        y = rng.normal(size=(case.batch, spec.dims[-1])).astype(np.float32)
    base = np.concatenate([np.concatenate([(rng.normal(size=(K, N)) / math.sqrt(K)).reshape(-1), 0.2 * rng.normal(size=N)])
                           for K, N in zip(spec.dims[:-1], spec.dims[1:])])
    gamma = 1.0 if case.median else case.g32
    # gamma d_ij^2 = u_i + u_j up to the draws: off-diagonal K between exp(-2.2) and exp(-0.3), every entry its own value
    u = np.array([0.5]) if M == 1 else (np.linspace(0.95, 1.05, M) if case.median else np.linspace(0.15, 1.1, M))
    if case.kind == "rep":
        assert spec.loss == "mse" and spec.acts[-1] == "linear"
        w = np.ones(D)
        w[last_layer(spec)] = 0.0
        base[last_layer(spec)] = 0.0     # output, delta and every loss gradient exactly zero
    elif case.kind == "coupled":
        # spread per layer block in proportion to the block's loss gradient, so that repulsion and drive stay comparable
        # in every block (clipped to a factor of twenty-five between blocks)
        _, g, _ = o_mlp.loss_and_grad(base, x, y, spec)
        w = np.empty(D)
        for _, sl in blocks(spec):
            top = max(np.abs(g[sl]).max(), BLOCK_FLOOR * np.abs(g).max())
            w[sl] = np.maximum(np.abs(g[sl]), ELEM_FLOOR * top)
    else:
        w = np.full(D, 0.02 * math.sqrt(D))
    # the deviations from the common centre: orthogonal directions (each still weighted element by element) of squared
    # length u_i / gamma, so that gamma d_ij^2 = u_i + u_j up to the float32 rounding of the particles
    q, _ = np.linalg.qr(w[:, None] * rng.normal(size=(D, M)))
    parts = base[None, :] + np.sqrt(u / gamma)[:, None] * q.T
    if case.kind == "drive" and M > 1:
        # far apart along a direction the softmax does not see: a common shift of the last layer's biases
        assert spec.acts[-1] == SM
        N = spec.dims[-1]
        parts[:, D - N:] += (np.arange(M) * math.sqrt(1000.0 / (gamma * N)))[:, None]
    if case.twin:
        parts[1] = parts[0]
    parts = parts.astype(np.float32)
    if not has_adam_step(case):
        z = np.zeros((case.nl, D), dtype=np.float32)
        return SvgdData(x, y, parts, z, z)
    phi = ref_sweep(case, SvgdData(x, y, parts, None, None), parts, None, None, 1)["phi"]
    scale = np.empty(D)
    for _, sl in blocks(spec):
        scale[sl] = np.abs(phi[:, sl]).max()
    assert scale.min() > 0
    m0 = (rng.choice([-1.0, 1.0], size=phi.shape) * rng.uniform(0.5, 1.0, size=phi.shape) * scale).astype(np.float32)
    v0 = (rng.uniform(0.25, 4.0, size=phi.shape) * scale * scale).astype(np.float32)
    return SvgdData(x, y, parts, m0, v0)


def dist_parts(case: SvgdCase) -> np.ndarray:
    """The particle matrix observable (a) runs on: the case's, with the all-zero last layer of a repulsion-only case filled
    (the last element of D must count in the distances)."""
    parts = _svgd_data(case).parts.copy()
    if case.kind == "rep":
        ll = last_layer(case.spec)
        rng = np.random.default_rng(case.D + case.M)
        parts[:, ll] = (0.05 * rng.normal(size=parts[:, ll].shape)).astype(np.float32)
    return parts


def svgd_data(case: SvgdCase) -> SvgdData:
    """Seeded inputs of a case (computed once per process and left unchanged)."""
    d = _svgd_data(case)
    for a in d:
        a.setflags(write=False)
    return d


# ---------------------------------------------------------------- one sweep, restated on oracle.svgd (any dtype, wrong variants)
MUTATIONS = [
    "repulsion with the wrong sign", "repulsion without the factor 2", "repulsion without gamma", "exp(-d) instead of exp(-gamma d)",
    "K row sum without the diagonal", "division by the local row count", "kernel row of il instead of row0 + il",
    "the last particle left out of the sums", "Gauss-Seidel evaluated as Jacobi", "Jacobi evaluated as Gauss-Seidel",
    "median over the off-diagonal entries only", "median as the upper middle value", "log(M) instead of log(M + 1)",
    "lr_t without bias correction", "Adam from zero state", "loss divided by the local row count",
]
DIST_MUTATION = "the last element of D left out of the distances"     # observable (a)
ADAM_MUTATIONS = ("lr_t without bias correction", "Adam from zero state")   # seen by observable (c) only


def mutation_applies(case: SvgdCase, mutation: str) -> bool:
    """Whether the wrong variant changes what the case computes (and the case runs wrong variants at all)."""
    if case.big:
        return False
    M, rep = case.M, case.kind in ("rep", "coupled") and case.M > 1
    if mutation in ("repulsion with the wrong sign", "repulsion without the factor 2"):
        return rep
    if mutation in ("repulsion without gamma", "exp(-d) instead of exp(-gamma d)"):
        return rep and not case.median
    if mutation == "K row sum without the diagonal":
        return case.kind in ("drive", "coupled")
    if mutation in ("division by the local row count", "loss divided by the local row count"):
        return case.shard and (case.kind != "rep" or mutation.startswith("division"))
    if mutation == "kernel row of il instead of row0 + il":
        return case.shard and case.row0 > 0 and rep
    if mutation == "the last particle left out of the sums":
        return rep and not case.median and case.row0 + case.nl < M + (not case.shard)
    if mutation == "Gauss-Seidel evaluated as Jacobi":
        return case.sweep == "gs" and rep
    if mutation == "Jacobi evaluated as Gauss-Seidel":
        return case.sweep == "jacobi" and rep and case.nl > 1 and not case.median
    if mutation.startswith("median") or mutation.startswith("log(M)"):
        return case.median
    if mutation in ADAM_MUTATIONS:
        return has_adam_step(case)
    raise KeyError(mutation)


def _median_h(sq: np.ndarray, M: int, mutation) -> float:
    """The bandwidth of oracle.svgd.median_kernel, or a wrong one."""
    if mutation == "median over the off-diagonal entries only":
        med = np.median(sq[~np.eye(M, dtype=bool)])
    elif mutation == "median as the upper middle value":
        med = np.sort(sq.reshape(-1))[(M * M) // 2]
    else:
        med = np.median(sq)
    return float(np.sqrt(0.5 * med / np.log(M if mutation == "log(M) instead of log(M + 1)" else M + 1)))


def _kernel_row(src: np.ndarray, i: int, gamma: float, mutation):
    if mutation is None:
        return o_svgd.rbf_row(src, i, gamma)
    diff = src[i][None, :] - src
    d2 = np.sum(diff * diff, axis=1)
    k = np.exp(-d2) if mutation == "exp(-d) instead of exp(-gamma d)" else np.exp(-gamma * d2)
    if mutation == "the last particle left out of the sums":
        k[-1] = 0.0
    f = {"repulsion with the wrong sign": -2.0 * gamma, "repulsion without the factor 2": gamma,
         "repulsion without gamma": 2.0}.get(mutation, 2.0 * gamma)
    return k, f * (k[:, None] * diff).sum(axis=0)


def lr_t(t: int, dt=np.float64, mutation=None, kernel_consts: bool = False):
    """Adam's step size as oracle.svgd.adam_update takes it in `dt`; kernel_consts: the float32 the library hands its
    kernels, (float)((double)lr sqrt(1 - 0.999^t) / (1 - 0.9^t)) of the float32 lr (in float32 the oracle's own 1 - 0.999^t
    loses five digits to cancellation, which no kernel does)."""
    if kernel_consts:
        lr = float(np.float32(LR))
        return dt(np.float32(lr if mutation == "lr_t without bias correction"
                             else lr * math.sqrt(1.0 - o_svgd.BETA2 ** t) / (1.0 - o_svgd.BETA1 ** t)))
    if mutation == "lr_t without bias correction":
        return dt(LR)
    return dt(LR) * np.sqrt(dt(1) - dt(o_svgd.BETA2) ** t) / (dt(1) - dt(o_svgd.BETA1) ** t)


def ref_sweep(case: SvgdCase, data: SvgdData, parts, m0, v0, t: int, dtype=np.float64, mutation=None, seen=None,
              kernel_consts: bool = False) -> dict:
    """One pyz_svgd_step of the case's local rows from the (M, D) matrix `parts` and the Adam state (m0, v0; None: zero) at
    step t, in `dtype`: the arithmetic of oracle.svgd.svgd_step (tests/test_svgd_dispatch_table.py holds the two equal,
    bit for bit, in float64 and float32), on a shard too, with `mutation` one of the wrong variants above.  `seen` (n_local,
    D): under Gauss-Seidel row i is evaluated against THESE values of the rows before it (a device's stored result)
    instead of this function's own, so that every row's bound is a bound on one row.  Returns phi, m, v, x (n_local, D),
    loss, and the terms the bounds need: k (n_local, M) float64 kernel rows, g the loss gradients, drive = sum_j K_ij g_i
    / M, rep = the repulsion / M, gamma the bandwidth used.  kernel_consts: Adam's 1 - beta as the kernels' float32 inputs
    (1.0f - 0.9f, 1.0f - 0.999f) instead of the oracle's dtype(1 - beta): what the comparisons use on both sides."""
    dt, spec, M, nl, row0 = dtype, case.spec, case.M, case.nl, case.row0
    c1, c2 = (dt(C1), dt(C2)) if kernel_consts else (dt(1 - o_svgd.BETA1), dt(1 - o_svgd.BETA2))
    P = np.asarray(parts, dtype=np.float64).copy()
    snap = P.copy()
    gs = (case.sweep == "gs") != (mutation in ("Gauss-Seidel evaluated as Jacobi", "Jacobi evaluated as Gauss-Seidel"))
    zero = np.zeros((nl, case.D), dtype=dt)
    if m0 is None or mutation == "Adam from zero state":
        m0, v0 = zero, zero
    m, v = np.array(m0, dtype=dt), np.array(v0, dtype=dt)
    out = {q: np.empty((nl, case.D)) for q in ("phi", "x", "g", "drive", "rep")}
    out["k"] = np.empty((nl, M))
    gamma = None if case.median else case.g32
    if case.median:
        assert not gs or mutation is not None
        if mutation in ("median over the off-diagonal entries only", "median as the upper middle value", "log(M) instead of log(M + 1)"):
            diff = snap[:, None, :] - snap[None, :, :]
            K_med, dx_med, h = o_svgd.median_kernel(snap, _median_h(np.sum(diff * diff, axis=-1), M, mutation))
        else:
            K_med, dx_med, h = o_svgd.median_kernel(snap)
        gamma = 0.5 / h ** 2
    total, div = 0.0, (nl if mutation == "division by the local row count" else M)
    for il in range(nl):
        i = row0 + il
        theta = P[i].astype(dt)
        loss, g, _ = o_mlp.loss_and_grad(theta, data.x, data.y, spec, dt)
        ir = il if mutation == "kernel row of il instead of row0 + il" else i
        if case.median:
            k, rep = K_med[ir], dx_med[ir]
            rep = {"repulsion with the wrong sign": -rep, "repulsion without the factor 2": 0.5 * rep}.get(mutation, rep)
        else:
            k, rep = _kernel_row(P if gs else snap, ir, gamma, mutation)
        kd = k.astype(dt)
        ks = kd.sum() - kd[ir] if mutation == "K row sum without the diagonal" else kd.sum()
        phi = (ks * g + rep.astype(dt)) / dt(div)
        g_ = np.asarray(phi, dtype=dt)
        m[il] = m[il] + (g_ - m[il]) * c1
        v[il] = v[il] + (g_ * g_ - v[il]) * c2
        new = theta - lr_t(t, dt, mutation, kernel_consts) * m[il] / (np.sqrt(v[il]) + dt(o_svgd.ADAM_EPS))
        P[i] = new.astype(np.float64) if seen is None else np.asarray(seen[il], dtype=np.float64)
        total += loss / (nl if mutation == "loss divided by the local row count" else M)
        out["phi"][il], out["x"][il], out["g"][il], out["k"][il] = phi, new, g, k
        out["drive"][il], out["rep"][il] = float(ks) * g.astype(np.float64) / div, rep / div
    out.update(m=m, v=v, loss=total, gamma=gamma)
    return out


def kernel_emulation(case: SvgdCase, data: SvgdData, parts, seen=None) -> dict:
    """Adam's first step from a zero state with phi rounded where the kernels round it (k_svgd_update_tile): K and the
    repulsion in float64, the latter as x_i sum_j K_ij - sum_j K_ij x_j, one rounding to float32, the row sum of K
    accumulated in float32, phi = (ksum g + rep) / M in float32.  What stands in for the device where the bound is a
    bound on roundings (the repulsion-only cases)."""
    f32 = np.float32
    P = np.asarray(parts, dtype=np.float64).copy()
    snap = P.copy()
    gamma = 0.5 / o_svgd.median_kernel(snap)[2] ** 2 if case.median else case.g32
    nl, M = case.nl, case.M
    phi = np.empty((nl, case.D), dtype=f32)
    x = np.empty_like(phi)
    total = 0.0
    for il in range(nl):
        i = case.row0 + il
        src = P if case.sweep == "gs" else snap      # (the rows before i as STORED: float32)
        diff = src[i][None, :] - src
        k = np.exp(-gamma * np.sum(diff * diff, axis=1))
        ksum = f32(0.0)
        for kj in k:
            ksum = f32(ksum + f32(kj))
        rep = (src[i] * float(np.sum(k)) - k @ src) * (2.0 * gamma)
        loss, g, _ = o_mlp.loss_and_grad(P[i].astype(f32), data.x, data.y, case.spec, f32)
        total += float(loss) / M
        phi[il] = (ksum * g.astype(f32) + rep.astype(f32)) / f32(M)
        m = (phi[il] * f32(C1)).astype(f32)
        vv = ((phi[il] * phi[il]).astype(f32) * f32(C2)).astype(f32)
        x[il] = P[i].astype(f32) - lr_t(1, f32, kernel_consts=True) * m / (np.sqrt(vv) + f32(1e-7))
        if case.sweep == "gs":
            P[i] = x[il] if seen is None else seen[il]
    m = (phi * f32(C1)).astype(f32)
    return dict(phi=phi, m=m, v=((phi * phi).astype(f32) * f32(C2)).astype(f32), x=x, loss=total)


def as_stored(out: dict) -> dict:
    """What a float32 device would leave of a reference sweep."""
    return {q: np.asarray(out[q], dtype=np.float32) for q in ("m", "v", "x", "loss")}


# ---------------------------------------------------------------- the comparisons
def _ratio(err, tol):
    err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(tol, 1e-300))))


def _within(err, tol, what):
    err, tol = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(tol, dtype=np.float64), np.shape(err))
    assert np.all(np.isfinite(err)), f"{what}: non-finite values"
    bad = err > tol
    if bad.any():
        i = np.unravel_index(int(np.argmax(err / np.maximum(tol, 1e-300))), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} elements outside the bound, worst at {tuple(map(int, i))}: "
                             f"error {err[i]:.3e} > {tol[i]:.3e}")
    return _ratio(err, tol)


def sq_distances(parts) -> np.ndarray:
    """sum_d (x_i - x_j)^2 in float64 on the float32 inputs (differences exact, squares rounded once, numpy's pairwise
    sums: an error below 2 (log2 D + 2) 2^-53 d^2, under a fiftieth of the bounds below for every D of the table)."""
    P = np.asarray(parts, dtype=np.float64)
    out = np.empty((P.shape[0], P.shape[0]))
    for i in range(P.shape[0]):
        diff = P[i][None, :] - P
        out[i] = np.sum(diff * diff, axis=1)
    return out


def compare_distances(parts, got, form: str, what: str = "") -> dict:
    """Observable (a): the (M, M) float64 matrix `got` against `sq_distances`.
    pairwise: |err_ij| <= 2 D 2^-53 d_ij^2 (D sums and D squares, each rounded once), the diagonal exactly 0;
    gram:     |err_ij| <= 2 D 2^-53 (|x_i|^2 + |x_j|^2) (products exact, the sums of the Gram entry and of the two norms round),
              the diagonal included;  both: d_ij == d_ji bit for bit."""
    P = np.asarray(parts, dtype=np.float64)
    M, D = P.shape
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (M, M)
    ref = sq_distances(P)
    assert np.array_equal(got.view(np.int64), got.T.copy().view(np.int64)), f"{what}: d_ij and d_ji differ in their bits"
    n2 = np.sum(P * P, axis=1)
    if form == "pairwise":
        assert np.all(np.diag(got) == 0.0), f"{what}: the diagonal of the pairwise form is not exactly zero"
        tol = 2.0 * D * 2.0 ** -53 * ref
    else:
        tol = 2.0 * D * 2.0 ** -53 * (n2[:, None] + n2[None, :])
    return {f"d2 {form}": _within(np.abs(got - ref), tol, f"{what}: squared distances, {form} form")}


def phi_tolerance(case: SvgdCase, ref: dict, parts, seen=None) -> np.ndarray:
    """The (n_local, D) bound on |phi_dev - phi64| of observable (b), by the kind of the case.
    rep:     2^-22 |phi64| (the float32 roundings of the repulsion, of the division by M and of Adam's m) +
             2^-50 2 gamma (|x_i| sum_j K_ij + sum_j K_ij |x_j|) / M (the float64 cancellation in x_i ksum - sum_j K_ij x_j) +
             2 gamma sum_j K_ij |x_i - x_j| (gamma e_ij + 2^-51) / M: the kernel values themselves, K_ij = exp(-gamma d_ij^2),
             carry the rounding of the device's float64 distances, e_ij = the bound of observable (a) for the form that ran
             (2 D 2^-53 d_ij^2 pairwise, 2 D 2^-53 (|x_i|^2 + |x_j|^2) through the Gram matrix), and of exp (two units in the
             last place).  Where the terms of the repulsion cancel, |phi64| is small and this is all the accuracy float64
             kernel values have: the first run of the matrix on the device missed the two-term bound on exactly those
             elements (profiles/svgd_matrix/rep_bound_before_k_term.log), by 1e-13 absolute on phi of 1e-4;
    drive:   1e-4 of the row's block scale (head_cases.close_blocks);
    coupled: per row and layer block 1e-4 (sum_j K_ij / M) max(max|g_block|, 1e-3 max|g|) + 2^-22 max_block(|drive| + |rep|)."""
    nl, M, spec = case.nl, case.M, case.spec
    phi = ref["phi"]
    if case.kind == "rep":
        P = np.abs(np.asarray(parts, dtype=np.float64))
        tol = np.empty_like(phi)
        for il in range(nl):
            Pa = P.copy()
            if case.sweep == "gs" and seen is not None:
                Pa[:il] = np.abs(np.asarray(seen[:il], dtype=np.float64))
            k, i = ref["k"][il], case.row0 + il
            tol[il] = 2.0 ** -22 * np.abs(phi[il]) + 2.0 ** -50 * 2.0 * ref["gamma"] * (Pa[i] * k.sum() + k @ Pa) / M
            Ps = np.asarray(parts, dtype=np.float64).copy()
            if case.sweep == "gs" and seen is not None:
                Ps[:il] = np.asarray(seen[:il], dtype=np.float64)
            diff = Ps[i][None, :] - Ps
            n2 = np.sum(Ps * Ps, axis=1)
            e = 2.0 * case.D * 2.0 ** -53 * (n2[i] + n2 if case.dist_form == "gram" else np.sum(diff * diff, axis=1))
            tol[il] += 2.0 * ref["gamma"] * ((k * (ref["gamma"] * e + 2.0 ** -51)) @ np.abs(diff)) / M
        return tol
    tol = np.empty_like(phi)
    for il in range(nl):
        for _, sl in blocks(spec):
            if case.kind == "drive":
                tol[il, sl] = 1e-4 * max(np.abs(phi[il, sl]).max(), 1e-3 * np.abs(phi[il]).max())
            else:
                g = np.abs(ref["g"][il])
                tol[il, sl] = (1e-4 * (ref["k"][il].sum() / M) * max(g[sl].max(), 1e-3 * g.max())
                               + 2.0 ** -22 * (np.abs(ref["drive"][il, sl]) + np.abs(ref["rep"][il, sl])).max())
    return tol


def ulps(a, b) -> np.ndarray:
    """|a - b| in units of the last place of the float32 values `a`."""
    a = np.asarray(a, dtype=np.float32)
    return np.abs(a.astype(np.float64) - np.asarray(b, dtype=np.float64)) / np.spacing(np.abs(a)).astype(np.float64)


# v against float32(phi_dev^2 (1.0f - 0.999f)) in units of v's last place: half a unit for v's own rounding, one for the
# rounding of phi^2 (2^-24 relative, a whole unit where v's mantissa is near 2) and two because m = float32(phi (1.0f -
# 0.9f)) gives phi_dev only to 2^-24 relative, doubled by the square.  (Two units, as first planned, leaves no room for
# the last term: float32 arithmetic itself, the kernel emulation below, reaches 2.7.)
V_ULPS = 3.5


def compare_phi(case: SvgdCase, data: SvgdData, got: dict, what: str = "") -> dict:
    """Observables (b) and (d) of Adam's first step from a zero state: `got` holds the float32 m, v, x (n_local, D) and the
    loss a device (or a stand-in) left.  From m = v = 0 at t = 1 the kernels leave m = phi (1.0f - 0.9f): phi_dev = m /
    (1.0f - 0.9f) reads phi element by element, whatever Adam then does with it; v must be float32(phi_dev^2 (1.0f -
    0.999f)) within two units in the last place.  The reference of row i is evaluated against the rows the device stored
    before it (Gauss-Seidel).  Returns quantity -> error over tolerance; raises AssertionError on the first bound missed.
    No element is exempt."""
    what = f"{what}{case.name}"
    seen = got["x"] if case.sweep == "gs" else None
    ref = ref_sweep(case, data, data.parts, None, None, 1, seen=seen, kernel_consts=True)
    m, v = np.asarray(got["m"], dtype=np.float32), np.asarray(got["v"], dtype=np.float32)
    phi_dev = m.astype(np.float64) / C1
    rep = {}
    if case.kind == "rep":
        ll = last_layer(case.spec)
        assert float(got["loss"]) == 0.0, f"{what}: loss {float(got['loss'])!r} of zero outputs against zero targets"
        assert np.all(m[:, ll] == 0) and np.all(v[:, ll] == 0), f"{what}: phi of the all-zero last layer is not exactly zero"
        assert np.all(ref["g"] == 0)
    tol = phi_tolerance(case, ref, data.parts, seen)
    rep["phi"] = _within(np.abs(phi_dev - ref["phi"]), tol, f"{what}: phi ({case.kind})")
    rep["v ulps"] = _within(ulps(v, phi_dev * phi_dev * C2), V_ULPS, f"{what}: v against float32(phi_dev^2 (1.0f - 0.999f)), in ulps")
    if case.kind != "rep":
        rep["loss"] = _within(abs(float(got["loss"]) - ref["loss"]), 1e-4 * abs(ref["loss"]), f"{what}: loss")
    return rep


def compare_adam(case: SvgdCase, data: SvgdData, got: dict, what: str = "", t: int = T_ADAM) -> dict:
    """Observable (c): one sweep at step t = 7 from the state (data.m0, data.v0) against the float64 restatement, with the
    tolerance of phi carried through Adam:
        dm = 0.1 dphi + 2^-23 max(|m0|, |m1|, |phi|)                 (three float32 roundings of terms no larger)
        dv = 0.002 |phi| dphi + 2^-21 max(v0, v1, phi^2)             (v's own rounding alone is 2^-24 v1 and, where phi is small
                                                                      beside sqrt v0, all there is: 2^-21 keeps a float32
                                                                      stand-in four times inside, as the table demands)
        dx = lr_t (dm / (sqrt v + 1e-7) + |m| dv / (2 sqrt v (sqrt v + 1e-7)^2)) + 2^-23 |x| + 2^-21 |step|
    with step = lr_t m / (sqrt v + 1e-7): its product, square root, sum and quotient round once each and lr_t is itself a
    float32 (five times 2^-24 of the step; without the term an element with x near zero has no allowance for them).
    The only place particles are compared.  Under Gauss-Seidel the reference of row i sees the device's rows 0 .. i - 1."""
    what = f"{what}{case.name} t={t}"
    seen = got["x"] if case.sweep == "gs" else None
    ref = ref_sweep(case, data, data.parts, data.m0, data.v0, t, seen=seen, kernel_consts=True)
    dphi = phi_tolerance(case, ref, data.parts, seen)
    phi, m1, v1, x1 = (np.abs(ref[q]) for q in ("phi", "m", "v", "x"))
    m0, v0 = np.abs(data.m0.astype(np.float64)), data.v0.astype(np.float64)
    dm = 0.1 * dphi + 2.0 ** -23 * np.maximum(np.maximum(m0, m1), phi)
    dv = 0.002 * phi * dphi + 2.0 ** -21 * np.maximum(np.maximum(v0, v1), phi * phi)
    sv = np.sqrt(v1)
    dx = (float(lr_t(t, kernel_consts=True)) * (dm / (sv + 1e-7) + m1 * dv / (2.0 * sv * (sv + 1e-7) ** 2)) + 2.0 ** -23 * x1
          + 2.0 ** -21 * float(lr_t(t, kernel_consts=True)) * m1 / (sv + 1e-7))
    rep = {"m1": _within(np.abs(got["m"].astype(np.float64) - ref["m"]), dm, f"{what}: m"),
           "v1": _within(np.abs(got["v"].astype(np.float64) - ref["v"]), dv, f"{what}: v"),
           "x1": _within(np.abs(got["x"].astype(np.float64) - ref["x"]), dx, f"{what}: particles"),
           "loss": _within(abs(float(got["loss"]) - ref["loss"]), 1e-4 * abs(ref["loss"]), f"{what}: loss")}
    return rep


def old_svgd_shapes():
    """The shapes the older SVGD tests run (tests/test_gpu_parity.py, test_gpu_baseline_shapes.py, test_gpu_svgd_shard.py,
    test_gpu_svgd_gs_resident.py), as cases of this table, for judging which cells they reach: name -> SvgdCase.  They
    all use gamma 1.0 or the median, aligned buffers, and compare forms with each other or whole steps with the oracle."""
    TC, MN = ((5, 7, 3), (R, SM), "scce"), ((784, 200, 10), (R, SM), "scce")
    g = 1.0
    return {
        "parity::test_svgd_step_matches_oracle[gauss_seidel]": _c("o1", TC, 5, 11, "gs", "coupled", g),
        "parity::test_svgd_step_matches_oracle[jacobi]": _c("o2", TC, 5, 11, "jacobi", "coupled", g),
        "parity::test_svgd_gauss_seidel_paths[2]": _c("o3", W, 7, 130, "gs", "coupled", g),
        "parity::test_svgd_gauss_seidel_paths[1]": _c("o4", W, 7, 130, "gs", "coupled", g, env=RES0),
        "parity::test_svgd_gauss_seidel_paths[0]": _c("o5", W, 7, 130, "gs", "coupled", g, env={"PYZ_SVGD_GS_FUSED": 0}),
        "parity::test_svgd_jacobi_shard_equals_whole": _c("o6", TC, 5, 11, "jacobi", "coupled", g, row0=2, n_local=3),
        "parity::test_svgd_jacobi_tiled_sweep[1]": _c("o7", W, 8, 130, "jacobi", "coupled", g),
        "parity::test_svgd_jacobi_tiled_sweep[1] shard": _c("o8", W, 8, 130, "jacobi", "coupled", g, row0=4, n_local=4),
        "parity::test_svgd_jacobi_tiled_sweep[0]": _c("o9", W, 8, 130, "jacobi", "coupled", g, env=PAIR),
        "parity::test_svgd_jacobi_tiled_sweep[0] shard": _c("o10", W, 8, 130, "jacobi", "coupled", g, row0=4, n_local=4, env=PAIR),
        "baseline_shapes::c5[gauss_seidel-resident]": _c("o11", MN, 64, 1024, "gs", "coupled", g),
        "baseline_shapes::c5[gauss_seidel-fused]": _c("o12", MN, 64, 1024, "gs", "coupled", g, env=RES0),
        "baseline_shapes::c5[gauss_seidel-rows]": _c("o13", MN, 64, 1024, "gs", "coupled", g, env={"PYZ_SVGD_GS_FUSED": 0}),
        "baseline_shapes::c5[jacobi-gram]": _c("o14", MN, 64, 1024, "jacobi", "coupled", g),
        "baseline_shapes::c5[jacobi-gram] shard": _c("o15", MN, 64, 1024, "jacobi", "coupled", g, row0=32, n_local=32),
        "baseline_shapes::c5[jacobi-pairwise]": _c("o16", MN, 64, 1024, "jacobi", "coupled", g, env=PAIR),
        "baseline_shapes::c5[jacobi-pairwise] shard": _c("o17", MN, 64, 1024, "jacobi", "coupled", g, row0=32, n_local=32, env=PAIR),
        "baseline_shapes::c5[jacobi-rows]": _c("o18", MN, 64, 1024, "jacobi", "coupled", g, env={"PYZ_SVGD_TILES": 0}),
        "baseline_shapes::median": _c("o19", MN, 64, 1024, "jacobi", "coupled", "median"),
        "baseline_shapes::median shard": _c("o20", MN, 64, 1024, "jacobi", "coupled", "median", row0=32, n_local=32),
        "gs_resident::equals_one_launch[tiny_m1]": _c("o21", TINY, 1, 90, "gs", "coupled", g),
        "gs_resident::equals_one_launch[tiny_m5-2]": _c("o22", TINY, 5, 90, "gs", "coupled", g, env=RES2),
        "gs_resident::equals_one_launch[wide3_m64-2]": _c("o23", W, 64, 90, "gs", "coupled", g, env=RES2),
        "gs_resident::equals_one_launch[wide3_m9] per launch": _c("o24", W, 9, 90, "gs", "coupled", g,
                                                                 env={"PYZ_SVGD_GS_RESIDENT": 0, "PYZ_SVGD_GS_ZIGZAG": 0}),
        "svgd_shard::shards of 16 of 64": _c("o25", W, 64, 64, "jacobi", "coupled", g, row0=16, n_local=16),
    }
