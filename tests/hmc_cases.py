"""The HMC case table and the dispatch it relies on (a plain module: imported by the HMC tests; no torch, no GPU).

`pyz_hmc_step` (csrc/pyz_api.hip, "H2-H5") picks one of four implementations from the shape, the chain count and a few
per-call switches.  This module restates that choice in plain Python (`dispatch`, `expected_path`), names the cells of
the coverage table (`CELLS`, `reached_cells`), lists cases that together reach every cell (`CASES`), draws their inputs
(`case_data`), runs the float64 / float32 oracle and its deliberately wrong variants on them (`oracle_result`,
`MUTATIONS`), derives the tolerances from the float32 oracle's own error (`tolerances`) and holds the one comparison
used everywhere (`compare`).  tests/test_hmc_dispatch_table.py pins the restatement to the source and checks on the CPU
that the comparison sees every wrong oracle; tests/test_gpu_hmc_matrix.py runs the cases on the kernels."""

from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import numpy as np

from oracle import hmc as o_hmc
from oracle import mlp as o_mlp
from oracle import philox as o_philox

# ---------------------------------------------------------------- dispatch rules (csrc/pyz_api.hip, pyz_hmc_step)
HF_MAXI, HF_MAXC = 8, 8          # pyz_hmc_fused.h: PYZ_HF_MAXI, PYZ_HF_MAXC
HF_WAVES, HM_WAVES = 16, 4       # PYZ_HF_WAVES (one workgroup per chain), PYZ_HM_WAVES (a row slice)
HM_MAXW = 32                     # pyz_hmc_multi.h: PYZ_HM_MAXW, slices per chain at most
ROWS_PER_WG = 96                 # default of PYZ_HMC_ROWS_PER_WG
MULTI_MAX_CHAINS = 16            # default of PYZ_HMC_MULTI_MAX_CHAINS
LDS_LIMIT = 150 * 1024           # one workgroup's data set / one slice must fit
LDS_ATTR = 64 * 1024             # above it the launcher raises hipFuncAttributeMaxDynamicSharedMemorySize
HIDDEN_MAX = 64                  # H + C <= 64: one lane per hidden unit and per output bias
STREAM_HMC = 2                   # pyz_rng.h: PYZ_STREAM_HMC; chain c draws from stream 2 + 16 c
PER_CALL_ENV = ("PYZ_HMC_FUSED", "PYZ_HMC_MULTI", "PYZ_HMC_RESIDENT", "PYZ_HMC_GRAPH")   # read per call: cases may set them
ENV_FORBIDDEN = ("PYZ_HMC_SPIN_LIMIT", "PYZ_HMC_ROWS_PER_WG", "PYZ_HMC_MULTI_MAX_CHAINS")  # stay at their defaults
ACT_ARMS = ("relu", "tanh", "sigmoid", "linear")   # the case arms of the three PICK switches (linear: default)
DEFAULT_CU = 256                 # compute units of an MI355X (the GPU test passes the device's own count)


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def bucket(I: int, C: int) -> int:
    """const int bucket = (I <= 2 && C <= 2) ? 0 : ((I <= 4 && C <= 4) ? 1 : 2); MIC = 2, 4, 8."""
    return 0 if (I <= 2 and C <= 2) else (1 if (I <= 4 and C <= 4) else 2)


def fused_lds_bytes(N: int, MI: int, MC: int, C: int, D: int, mse: bool) -> int:
    """pyz_hmc_fused_lds_bytes."""
    fl = (4 + HF_WAVES) * D + 64 * (MI + MC + 2) + N * MI + N * MC + N * (C if mse else 1)
    return (fl * 4 + 15) // 16 * 16 + 64 * 8


def multi_lds_bytes(max_rows: int, MI: int, MC: int, C: int, D: int, mse: bool) -> int:
    """pyz_hmc_multi_lds_bytes."""
    fl = (3 + HM_WAVES) * D + 64 * (MI + MC + 2) + max_rows * MI + max_rows * MC + max_rows * (C if mse else 1)
    return (fl * 4 + 15) // 16 * 16 + 64 * 8


def n_params(dims) -> int:
    return sum((i + 1) * o for i, o in zip(dims[:-1], dims[1:]))


class Path(NamedTuple):
    path: str            # fused | multi | resident | generic
    bucket: Optional[int]
    NW: int              # slices per chain (0 when not sliced)
    slices: tuple        # rows of each slice
    launches: tuple      # the HMC launch sites of one call, in order, as KernelProbe names them
    graph: bool          # replayed from a captured graph when the call is on a side stream
    lds: int             # bytes of the one-workgroup form (0: not a two-layer model)
    mlds: int            # bytes of a slice workgroup


def dispatch(dims, acts, loss, rows, P, L, vec_prior=False, env=None, cu_count=DEFAULT_CU) -> Path:
    """The choice pyz_hmc_step makes, and the launches that follow from it."""
    env = env or {}
    flag = lambda k: int(env.get(k, 1))
    two = len(dims) == 3
    I, H, C = dims[0], dims[1], (dims[2] if two else 0)
    D, mse = n_params(dims), loss == "mse"
    b = bucket(I, C)
    MIC = (2, 4, 8)[b]
    lds = fused_lds_bytes(rows, MIC, MIC, C, D, mse) if two else 0
    NW = min(HM_MAXW, rows // max(16, ROWS_PER_WG))
    mlds = multi_lds_bytes(cdiv(rows, max(NW, 1)) + 1, MIC, MIC, C, D, mse) if two else 0
    multi_ok = bool(flag("PYZ_HMC_MULTI") and NW >= 2 and P <= MULTI_MAX_CHAINS and mlds <= LDS_LIMIT)
    small = bool(flag("PYZ_HMC_FUSED") and not vec_prior and two and I <= HF_MAXI and C <= HF_MAXC and H + C <= HIDDEN_MAX and
                 (lds <= LDS_LIMIT or multi_ok) and acts[0] != "softmax")
    if not small:
        seq = ["k_hmc_begin", "k_loss_finalize", "k_hmc_energy_finalize", "k_hmc_kick_drift"]
        seq += ["k_loss_finalize", "k_hmc_kick_drift"] * L
        seq += ["k_hmc_end_energy", "k_hmc_energy_finalize", "k_hmc_accept", "k_hmc_restore"]
        return Path("generic", None, 0, (), tuple(seq), False, lds, mlds)
    if not multi_ok:
        return Path("fused", b, 0, (), ("kern",), False, lds, mlds)
    slices = tuple(rows * (w + 1) // NW - rows * w // NW for w in range(NW))
    graph = bool(flag("PYZ_HMC_GRAPH"))
    if flag("PYZ_HMC_RESIDENT") != 0 and NW * P <= cu_count:
        return Path("resident", b, NW, slices, ("kres",), graph, lds, mlds)
    return Path("multi", b, NW, slices, ("kmulti",) * (L + 1) + ("k_hmc_multi_final",), graph, lds, mlds)


HMC_SITES = frozenset(["kern", "kmulti", "kres", "k_hmc_multi_final", "k_hmc_begin", "k_hmc_kick_drift", "k_hmc_end_energy",
                       "k_hmc_energy_finalize", "k_hmc_accept", "k_hmc_restore", "k_loss_finalize"])


# ---------------------------------------------------------------- cases
class HmcCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str
    rows: int
    P: int
    L: int
    eps: float
    m: float = 0.5
    prior: tuple = (0.0, 1.0)   # scalar prior (mean, sigma); sigma < 0: NaN potential
    vec_prior: bool = False     # per-element prior mean / sigma vectors instead (generic path only)
    momentum: str = "injected"  # injected (unit_p given) | philox (the library draws it)
    step: int = 0
    seed: int = 1
    env: dict = {}
    reject0: bool = False       # chain 0 rejected (by default even chains are accepted, odd ones rejected)

    @property
    def spec(self) -> o_mlp.MLPSpec:
        return o_mlp.MLPSpec(self.dims, self.acts, self.loss)

    @property
    def D(self) -> int:
        return n_params(self.dims)


def expected_path(case: HmcCase, cu_count: int = DEFAULT_CU, P: Optional[int] = None) -> Path:
    return dispatch(case.dims, case.acts, case.loss, case.rows, case.P if P is None else P, case.L, case.vec_prior,
                    case.env, cu_count)


def check_chains(P: int):
    """The chains a case compares with the oracle: all of up to four, else the first, the middle and the last."""
    return list(range(P)) if P <= 4 else sorted({0, (P // 2) | 1, P - 1})   # (the middle one odd: a rejected chain)


SMALL = ("fused", "multi", "resident")
PATHS = SMALL + ("generic",)
HEADS = ("scce", "mse linear", "mse tanh", "mse sigmoid")

CELLS = frozenset(
    [f"{p} <{w},{w}> {a}" for p in SMALL for w in (2, 4, 8) for a in ACT_ARMS] +
    [f"{p} head {h}" for p in SMALL for h in HEADS] +
    [f"{p} L={L}" for p in PATHS for L in (0, 1, 2, 20)] +
    [f"{p} momentum {mo}" for p in PATHS for mo in ("injected", "philox")] +
    [f"{p} prior mean!=0 sigma!=1" for p in PATHS] +
    ["C=1", "C=8", "I=1", "I=8", "H=1", "H=56 C=8", "H+C=65 generic", "I=9 generic", "C=9 generic",
     "chains=1", "chains=3", "chains=16 sliced", "chains=17 fused rows>=192", "chains>64 fused", "chains>64 generic",
     "rows=191 fused", "rows=192 NW=2", "rows%NW=1", "rows%NW=NW-1", "NW=17", "NW=32", "NW*P=CU resident", "NW*P>CU multi no env",
     "lds just under 150K MULTI=0 fused", "lds just over 150K MULTI=0 generic", "sliced mlds>64K",
     "generic three layers", "generic vec prior two layers", "generic D%4=1", "generic D%4=2", "generic D%4=3",
     "generic D=255", "generic D=256", "generic D=257", "generic D>1024", "generic scce", "generic mse",
     "generic FUSED=0 fused-eligible", "philox step>0 chains>1 D%4!=0", "prior sigma<0", "sliced GRAPH=0",
     "outcome accepted", "outcome rejected", "outcome burning"])


def head_of(case: HmcCase) -> str:
    return "scce" if case.loss == "scce" else f"mse {case.acts[-1]}"


def reached_cells(case: HmcCase, cu_count: int = DEFAULT_CU) -> set:
    """The cells a case reaches, from the dispatch restatement alone."""
    pa = expected_path(case, cu_count)
    p, dims, D, P, rows = pa.path, case.dims, case.D, case.P, case.rows
    cells = {f"{p} L={case.L}", f"{p} momentum {case.momentum}", f"chains={P}", "outcome burning"}
    two = len(dims) == 3
    if p in SMALL:
        w = (2, 4, 8)[pa.bucket]
        cells |= {f"{p} <{w},{w}> {case.acts[0]}", f"{p} head {head_of(case)}"}
        cells |= {f"C={dims[2]}", f"I={dims[0]}", f"H={dims[1]}"}
        if dims[1] == 56 and dims[2] == 8:
            cells.add("H=56 C=8")
    if case.prior[0] != 0.0 and case.prior[1] not in (1.0,) and case.prior[1] > 0 and not case.vec_prior:
        cells.add(f"{p} prior mean!=0 sigma!=1")
    if case.prior[1] < 0:
        cells.add("prior sigma<0")
    else:
        flags = [(c % 2 == 0) != (case.reject0 and c == 0) for c in range(P)]
        cells |= {"outcome accepted"} if any(flags) else set()
        cells |= {"outcome rejected"} if not all(flags) else set()
    if pa.NW:
        cells |= {f"NW={pa.NW}", "chains=16 sliced" if P == 16 else ""}
        if rows == 192 and pa.NW == 2:
            cells.add("rows=192 NW=2")
        if pa.NW > 2 and rows % pa.NW == 1:
            cells.add("rows%NW=1")
        if pa.NW > 2 and rows % pa.NW == pa.NW - 1:
            cells.add("rows%NW=NW-1")
        if pa.NW * P == cu_count and p == "resident":
            cells.add("NW*P=CU resident")
        if pa.NW * P > cu_count and p == "multi" and not case.env:
            cells.add("NW*P>CU multi no env")
        if pa.mlds > LDS_ATTR:
            cells.add("sliced mlds>64K")
        if case.env.get("PYZ_HMC_GRAPH") == "0":
            cells.add("sliced GRAPH=0")
    if p == "fused":
        if rows == 191:
            cells.add("rows=191 fused")
        if P == 17 and rows >= 2 * ROWS_PER_WG:
            cells.add("chains=17 fused rows>=192")
        if P > 64:
            cells.add("chains>64 fused")
        if case.env.get("PYZ_HMC_MULTI") == "0" and pa.lds <= LDS_LIMIT < dispatch(
                dims, case.acts, case.loss, rows + 1, P, case.L, False, case.env, cu_count).lds:
            cells.add("lds just under 150K MULTI=0 fused")
    if p == "generic":
        cells |= {f"generic D%4={D % 4}", f"generic D={D}", f"generic {case.loss}"}
        if D > 1024:
            cells.add("generic D>1024")
        if P > 64:
            cells.add("chains>64 generic")
        if not two:
            cells.add("generic three layers")
        elif case.vec_prior:
            cells.add("generic vec prior two layers")
        elif dims[1] + dims[2] == HIDDEN_MAX + 1 and dims[0] <= HF_MAXI and dims[2] <= HF_MAXC:
            cells.add("H+C=65 generic")
        elif dims[0] == HF_MAXI + 1 and dims[2] <= HF_MAXC and dims[1] + dims[2] <= HIDDEN_MAX:
            cells.add("I=9 generic")
        elif dims[2] == HF_MAXC + 1 and dims[0] <= HF_MAXI and dims[1] + dims[2] <= HIDDEN_MAX:
            cells.add("C=9 generic")
        if two and not case.vec_prior and case.env.get("PYZ_HMC_FUSED") == "0" and \
                expected_path(case._replace(env={}), cu_count).path != "generic":
            cells.add("generic FUSED=0 fused-eligible")
        if two and case.env.get("PYZ_HMC_MULTI") == "0" and pa.lds > LDS_LIMIT >= dispatch(
                dims, case.acts, case.loss, rows - 1, P, case.L, False, case.env, cu_count).lds:
            cells.add("lds just over 150K MULTI=0 generic")
    if case.momentum == "philox" and case.step > 0 and P > 1 and D % 4:
        cells.add("philox step>0 chains>1 D%4!=0")
    return cells & CELLS


R, T, G, LN, SM = "relu", "tanh", "sigmoid", "linear", "softmax"
SC, MS = "scce", "mse"
INJ, PHX = "injected", "philox"
NO_MULTI, NO_RES, NO_FUSED = {"PYZ_HMC_MULTI": "0"}, {"PYZ_HMC_RESIDENT": "0"}, {"PYZ_HMC_FUSED": "0"}
PRIOR2 = (0.15, 0.7)             # mean != 0, sigma != 1
BIG_LDS_CASE = "res_b2_linear_mlds_over_64k"   # the one case above 8192 rows (see its line)


def _c(name, dims, acts, loss, rows, P, L, eps, momentum=INJ, prior=(0.0, 1.0), m=0.5, vec_prior=False, step=0, seed=1, env=None,
       reject0=False):
    eps = float(np.float32(eps))   # the library takes a float: the oracle gets the same number
    return HmcCase(name, tuple(dims), tuple(acts), loss, rows, P, L, eps, m, tuple(prior), vec_prior, momentum, step, seed,
                   dict(env or {}), reject0)


CASES = [
    # ---- k_hmc_fused: fewer than 192 rows, more than 16 chains, or PYZ_HMC_MULTI=0
    _c("fused_b0_relu_rows191", (2, 50, 2), (R, SM), SC, 191, 3, 5, 0.02, m=0.1),
    _c("fused_b0_tanh_i1_h1_c1", (1, 1, 1), (T, LN), MS, 40, 1, 1, 0.07, PHX, m=0.1, step=2),
    _c("fused_b0_sigmoid_17_chains", (2, 10, 2), (G, T), MS, 192, 17, 2, 0.05, PHX, step=5, prior=PRIOR2),
    _c("fused_b0_linear_l0", (2, 7, 1), (LN, G), MS, 150, 2, 0, 0.1),
    _c("fused_b1_relu_l20_philox", (4, 30, 3), (R, SM), SC, 120, 3, 20, 0.03, PHX, step=3, prior=PRIOR2),
    _c("fused_b1_tanh_80_chains", (3, 5, 4), (T, SM), SC, 64, 80, 1, 0.07),
    _c("fused_b1_sigmoid_multi_off", (4, 12, 3), (G, LN), MS, 500, 2, 2, 0.03, env=NO_MULTI),
    _c("fused_b1_linear_l0_rejected", (3, 20, 4), (LN, T), MS, 96, 1, 0, 0.1, reject0=True),
    _c("fused_b2_relu_lds_under", (8, 56, 8), (R, SM), SC, 1054, 2, 3, 0.001, m=0.02, env=NO_MULTI),
    _c("fused_b2_tanh_mse_sigmoid", (5, 20, 8), (T, G), MS, 130, 3, 2, 0.07, PHX, step=1),
    _c("fused_b2_sigmoid_l20", (8, 16, 2), (G, SM), SC, 191, 4, 20, 0.05),
    _c("fused_b2_linear_neg_sigma", (2, 9, 5), (LN, SM), SC, 77, 3, 0, 0.05, prior=(0.0, -1.0)),
    # ---- k_hmc_resident: at least 192 rows, at most 16 chains, NW x chains workgroups within the chip
    _c("res_b0_relu_c3", (2, 50, 2), (R, SM), SC, 1600, 1, 20, 0.01, PHX, step=4),
    _c("res_b0_tanh_rows192", (2, 50, 2), (T, SM), SC, 192, 3, 1, 0.01, m=0.02),
    _c("res_b0_sigmoid_i1_rem1", (1, 8, 2), (G, SM), SC, 289, 2, 2, 0.03, m=0.1, prior=PRIOR2),
    _c("res_b0_linear_16_chains", (2, 6, 2), (LN, SM), SC, 479, 16, 2, 0.015, PHX, m=0.1, step=7),
    _c("res_b1_sigmoid_17_slices", (4, 30, 3), (G, SM), SC, 1640, 3, 6, 0.015),
    _c("res_b1_tanh_mse_tanh_l20", (3, 5, 2), (T, T), MS, 301, 2, 20, 0.05),
    _c("res_b1_relu_nw32_equals_cu", (4, 30, 3), (R, SM), SC, 3100, 8, 6, 0.005, PHX, step=1),
    _c("res_b1_linear_rows193", (4, 30, 3), (LN, LN), MS, 193, 3, 3, 0.03, prior=PRIOR2),
    _c("res_b2_relu_h56_c8", (8, 56, 8), (R, SM), SC, 1000, 1, 2, 0.007, reject0=True),
    _c("res_b2_tanh_mse_sigmoid", (8, 40, 8), (T, G), MS, 400, 2, 1, 0.07, PHX, m=0.1, step=9),
    _c("res_b2_sigmoid_nw32_l0", (8, 56, 8), (G, SM), SC, 3100, 1, 0, 0.007),
    _c("res_b2_linear_scce", (6, 10, 5), (LN, SM), SC, 700, 5, 2, 0.015),
    _c("res_b0_relu_16x16_equals_cu", (2, 8, 2), (R, SM), SC, 1540, 16, 3, 0.01, m=0.1),
    _c("res_b1_relu_graph_off", (3, 9, 3), (R, SM), SC, 400, 2, 2, 0.02, env={"PYZ_HMC_GRAPH": "0"}),
    _c("res_b0_tanh_neg_sigma", (2, 12, 2), (T, SM), SC, 300, 2, 1, 0.03, m=0.1, prior=(0.0, -1.0)),
    # 11 360 rows: with 96 rows per slice and at most 32 slices, the widest model (D = 960, 24 floats per row) needs
    # 355 rows per slice before a slice's LDS passes 64 KB; the only case above 8192 rows
    _c(BIG_LDS_CASE, (8, 56, 8), (LN, LN), MS, 11360, 1, 4, 0.005),
    # ---- k_hmc_multi + k_hmc_multi_final: PYZ_HMC_RESIDENT=0, or more workgroups than compute units
    _c("multi_b0_relu_over_cu", (2, 8, 2), (R, SM), SC, 1640, 16, 3, 0.02),
    _c("multi_b0_tanh_l0", (2, 50, 2), (T, SM), SC, 700, 3, 0, 0.02, env=NO_RES),
    _c("multi_b0_sigmoid_mse_sigmoid", (2, 10, 1), (G, G), MS, 290, 2, 2, 0.1, PHX, step=3, env=NO_RES),
    _c("multi_b0_linear_l20", (1, 6, 2), (LN, SM), SC, 250, 1, 20, 0.05, env=NO_RES, prior=PRIOR2),
    _c("multi_b1_relu_17_slices", (4, 30, 3), (R, SM), SC, 1650, 3, 2, 0.005, m=0.1, env=NO_RES),
    _c("multi_b1_tanh_mse_linear", (3, 5, 2), (T, LN), MS, 301, 2, 4, 0.03, env=NO_RES),
    _c("multi_b1_sigmoid_nw32", (4, 30, 3), (G, SM), SC, 3100, 3, 6, 0.002, m=0.02, env=NO_RES),
    _c("multi_b1_linear_mse_tanh", (4, 12, 4), (LN, T), MS, 479, 2, 2, 0.03, PHX, step=2, env=NO_RES),
    _c("multi_b2_relu_h56_c8", (8, 56, 8), (R, SM), SC, 1000, 2, 3, 0.005, env=NO_RES),
    _c("multi_b2_tanh_16_chains", (5, 20, 8), (T, SM), SC, 400, 16, 2, 0.02, env=NO_RES),
    _c("multi_b2_sigmoid_i8", (8, 16, 2), (G, SM), SC, 1000, 3, 4, 0.03, env=NO_RES),
    _c("multi_b2_linear_graph_off", (6, 10, 5), (LN, LN), MS, 600, 3, 1, 0.007, m=0.02,
       env={"PYZ_HMC_RESIDENT": "0", "PYZ_HMC_GRAPH": "0"}),
    # ---- the generic sequence around the Dense kernels
    _c("gen_three_layers", (4, 10, 6, 3), (T, R, SM), SC, 200, 3, 2, 0.03),
    _c("gen_vec_prior_two_layers", (2, 50, 2), (R, SM), SC, 300, 3, 3, 0.02, vec_prior=True),
    _c("gen_d255_fused_off", (2, 42, 3), (T, SM), SC, 150, 3, 2, 0.05, PHX, step=6, env=NO_FUSED),
    _c("gen_d256_fused_off_l0", (2, 36, 4), (R, LN), MS, 400, 2, 0, 0.05, env=NO_FUSED),
    _c("gen_d257_l20", (2, 51, 2), (G, SM), SC, 120, 2, 20, 0.03, env=NO_FUSED, prior=PRIOR2),
    _c("gen_d1210_i9_c10", (9, 60, 10), (R, SM), SC, 256, 3, 1, 0.02, PHX, step=1),
    _c("gen_i9", (9, 20, 4), (T, SM), SC, 128, 2, 1, 0.01, m=0.1),
    _c("gen_h_plus_c_65", (4, 57, 8), (T, SM), SC, 200, 2, 2, 0.01, m=0.02),
    _c("gen_c9", (3, 12, 9), (G, LN), MS, 100, 1, 2, 0.1),
    _c("gen_70_chains", (3, 8, 3, 2), (R, T, LN), MS, 64, 70, 1, 0.015, m=0.02),
    _c("gen_lds_over", (8, 56, 8), (R, SM), SC, 1055, 2, 3, 0.005, env=NO_MULTI),
    _c("gen_neg_sigma", (4, 10, 6, 3), (T, T, SM), SC, 90, 2, 1, 0.05, prior=(0.0, -2.0)),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"


# ---------------------------------------------------------------- data
class Data(NamedTuple):
    x: np.ndarray            # (rows, I) float32
    y: np.ndarray            # int32 labels / float32 targets
    q0: np.ndarray           # (P, D) float32
    z: np.ndarray            # (P, D) float32: the N(0,1) momentum draw of every chain
    prior_mu: object         # float, or (D,) float32
    prior_sigma: object


def philox_z(case: HmcCase, chain: int, step: Optional[int] = None, stream_chain: Optional[int] = None) -> np.ndarray:
    """The library's own momentum draw of a chain: stream PYZ_STREAM_HMC + 16 * chain, counter = the step."""
    c = chain if stream_chain is None else stream_chain
    return o_philox.normal(case.seed, STREAM_HMC + 16 * c, case.step if step is None else step, case.D).astype(np.float32)


def case_data(case: HmcCase) -> Data:
    """Seeded inputs of a case.  Inputs are standard normal; every layer of chain 0's q is scaled so that its
    pre-activations have an rms of 0.8 (tanh and sigmoid out of saturation, relu units alive), and the other chains
    start a few percent away from it.  Labels are drawn from chain 0's own model (classes from its softmax, targets =
    its output plus noise): the gradient is then the sampling noise of the rows, of the order sqrt(rows), not a bias
    of the order rows -- with purely random labels no step size keeps |log_ratio| small and moves q by more than
    float32 rounding at once."""
    spec = case.spec
    rng = np.random.default_rng(sum(map(ord, case.name)) + 7919 * case.seed)
    x = rng.normal(size=(case.rows, spec.dims[0])).astype(np.float32)
    parts, h = [], x.astype(np.float64)
    for (fan_in, fan_out), act in zip(zip(spec.dims[:-1], spec.dims[1:]), spec.acts):
        w = rng.normal(size=(fan_in, fan_out))
        b = rng.normal(size=fan_out) * 0.3
        zz = h @ w + b
        s = 0.8 / np.sqrt(np.mean(zz * zz))
        parts += [(w * s).reshape(-1), b * s]
        h = o_mlp._act(zz * s, act)
    base = np.concatenate(parts)
    q0 = np.empty((case.P, case.D), dtype=np.float32)
    q0[0] = base
    for c in range(1, case.P):
        q0[c] = base * (1.0 + 0.02 * rng.normal(size=case.D)) + 0.004 * rng.normal(size=case.D)
    if case.loss == "scce":
        cum = np.cumsum(h, axis=1)
        y = np.minimum((rng.uniform(size=(case.rows, 1)) > cum).sum(axis=1), spec.dims[-1] - 1).astype(np.int32)
    else:
        y = (h + 0.3 * rng.normal(size=h.shape)).astype(np.float32)
    if case.momentum == "philox":
        z = np.stack([philox_z(case, c) for c in range(case.P)])
    else:
        z = rng.normal(size=(case.P, case.D)).astype(np.float32)
    if case.vec_prior:
        mu = (rng.normal(size=case.D) * 0.1).astype(np.float32)
        sg = rng.uniform(0.6, 1.4, size=case.D).astype(np.float32)
    else:
        mu, sg = float(np.float32(case.prior[0])), float(np.float32(case.prior[1]))
    return Data(x, y, q0, z, mu, sg)


def hidden_stats(case: HmcCase, data: Data):
    """Over the checked chains, per hidden layer: (least share of pre-activations within +-4, largest share of units
    whose output is zero over the whole data set)."""
    spec = case.spec
    within, dead = [1.0] * (spec.n_layers - 1), [0.0] * (spec.n_layers - 1)
    for c in check_chains(case.P):
        h = data.x.astype(np.float64)
        for l, ((w, b), act) in enumerate(zip(o_mlp.unpack(data.q0[c].astype(np.float64), spec), spec.acts[:-1])):
            zz = h @ w + b
            h = o_mlp._act(zz, act)
            within[l] = min(within[l], float(np.mean(np.abs(zz) <= 4.0)))
            dead[l] = max(dead[l], float(np.mean(np.all(h == 0.0, axis=0))))
    return within, dead


# ---------------------------------------------------------------- the oracle and its wrong variants
MUTATIONS = ("drop_last_row", "drop_last_row_of_first_slice", "zero_last_hidden_unit", "zero_last_bias_grad", "no_prior_in_dU",
             "n_train_minus_1", "zero_last_momentum", "philox_chain0_stream")


def mutation_applies(case: HmcCase, mutation: str, chain: int) -> bool:
    if mutation == "drop_last_row_of_first_slice":
        return expected_path(case).NW >= 2
    if mutation == "philox_chain0_stream":
        return case.momentum == "philox" and chain > 0
    return True


def _hidden_unit_indices(spec: o_mlp.MLPSpec):
    """Flat indices of everything that belongs to the last unit of the last hidden layer."""
    l = spec.n_layers - 2
    (ko, bo), (ko2, _) = spec.offsets()[l], spec.offsets()[l + 1]
    K, N, N2 = spec.dims[l], spec.dims[l + 1], spec.dims[l + 2]
    return np.concatenate([ko + np.arange(K) * N + (N - 1), [bo + N - 1], ko2 + (N - 1) * N2 + np.arange(N2)])


def _mutated_potential(case: HmcCase, mutation: str):
    spec = case.spec
    pa = expected_path(case)
    keep = None
    if mutation == "drop_last_row":
        keep = np.arange(case.rows - 1)
    elif mutation == "drop_last_row_of_first_slice":
        keep = np.delete(np.arange(case.rows), pa.slices[0] - 1)
    hid = _hidden_unit_indices(spec) if mutation == "zero_last_hidden_unit" else None

    def potential(q, X, y, spec_, prior_mu, prior_sigma, n_train, dtype=np.float64):
        q = np.asarray(q, dtype=dtype)
        loss, g, _ = o_mlp.loss_and_grad(q, X, y, spec_, dtype)
        n_eff = n_train
        if keep is not None:    # the rows' gradients are summed, so a missing row is missing from the sum
            _, gk, _ = o_mlp.loss_and_grad(q, X[keep], y[keep], spec_, dtype)
            g = gk * dtype(len(keep) / n_train)
        if hid is not None:
            g = g.copy()
            g[hid] = 0
        if mutation == "zero_last_bias_grad":
            g = g.copy()
            g[-1] = 0
        if mutation == "n_train_minus_1":
            n_eff = n_train - 1
        mu = np.broadcast_to(np.asarray(prior_mu, dtype=dtype), q.shape)
        sg = np.broadcast_to(np.asarray(prior_sigma, dtype=dtype), q.shape)
        U = -o_hmc.normal_log_prob(q, mu, sg).sum() + loss * n_eff
        dU = g * n_eff
        if mutation != "no_prior_in_dU":
            dU = (q - mu) / (sg * sg) + dU
        return U, loss, dU
    return potential


def uniforms(case: HmcCase, data: Data):
    """One uniform per chain, placed as test_hmc_step_matches_oracle places them: half the float64 oracle's acceptance
    ratio (accepted) for even chains, twice it plus 0.1 (rejected) for odd ones, so rounding cannot flip a decision."""
    return _uniforms(case.name)


@functools.lru_cache(maxsize=None)
def _uniforms(name: str):
    case = CASE_BY_NAME[name]
    data = case_data(case)
    us = []
    for c in range(case.P):
        lr = _hmc(case, data, c, data.z[c], 0.5, False, np.float64)["log_ratio"]
        ratio = math.exp(min(lr, 50.0)) if np.isfinite(lr) else 0.5
        accept = (c % 2 == 0) != (case.reject0 and c == 0)
        us.append(float(np.float32(0.5 * ratio if accept else 2.0 * ratio + 0.1)))
    return tuple(us)


def _hmc(case, data, chain, z, u, burning, dtype, q=None):
    return o_hmc.hmc_step(data.q0[chain] if q is None else q, z, data.x, data.y, case.spec, data.prior_mu, data.prior_sigma,
                          case.L, case.eps, case.m, u=u, burning=burning, dtype=dtype)


def result_from(case, q0, z, burn, metro):
    """The compared quantities of one chain from a burning and a Metropolis run (oracle dicts, or the same keys from
    the library's q and stats)."""
    return dict(q0=np.asarray(q0), z=np.asarray(z), q_proposed=np.asarray(burn["q"]), loss_proposed=float(burn["loss"]),
                accepted=bool(metro["accepted"]), q=np.asarray(metro["q"]), loss=float(metro["loss"]),
                U0=float(metro["U0"]), K0=float(metro["K0"]), U1=float(metro["U1"]), K1=float(metro["K1"]),
                log_ratio=float(metro["log_ratio"]))


def oracle_result(case: HmcCase, data: Data, chain: int, dtype=np.float64, mutation: Optional[str] = None, u=None, q=None,
                  z=None):
    """oracle.hmc.hmc_step on one chain: a burning and a Metropolis run.  `mutation` makes it one of the wrong oracles."""
    z = data.z[chain] if z is None else z
    u = uniforms(case, data)[chain] if u is None else u
    z_run = z
    saved = o_hmc.potential_energy
    try:
        if mutation == "zero_last_momentum":
            z_run = z.copy()
            z_run[-1] = 0.0
        elif mutation == "philox_chain0_stream":
            z_run = philox_z(case, chain, stream_chain=0)
        elif mutation is not None:
            o_hmc.potential_energy = _mutated_potential(case, mutation)
        burn = _hmc(case, data, chain, z_run, u, True, dtype, q)
        metro = _hmc(case, data, chain, z_run, u, False, dtype, q)
    finally:
        o_hmc.potential_energy = saved
    return result_from(case, data.q0[chain] if q is None else q, z, burn, metro)


# ---------------------------------------------------------------- the comparison
F32_EPS = 2.0 ** -23
CAP = 1e-4          # the project's bound everywhere else: never looser than this
FACTOR = 8.0        # over the float32 oracle's own error: summation order (16 waves, up to 32 slices)
SCALARS = ("K1", "U1", "U0", "K0", "loss", "loss_proposed", "log_ratio")


def blocks(spec: o_mlp.MLPSpec):
    """(name, slice) of each layer's W and b block in the flat vector."""
    out = []
    for l, ((ko, bo), K, N) in enumerate(zip(spec.offsets(), spec.dims[:-1], spec.dims[1:])):
        out += [(f"W{l + 1}", slice(ko, ko + K * N)), (f"b{l + 1}", slice(bo, bo + N))]
    return out


def gradient_move(res, case: HmcCase) -> np.ndarray:
    """(q_proposed - q0) - L eps z in float64 from the stored float32 values: what the kernels' gradients moved q by."""
    f = lambda a: np.asarray(a).astype(np.float64)
    return (f(res["q_proposed"]) - f(res["q0"])) - case.L * case.eps * f(res["z"])


def quantities(res, ref, case: HmcCase):
    """{name: (value, reference, scale, floor)} of one chain.  The scale is the reference's own; the floor is the
    float32 rounding of what is stored."""
    out = {}
    energy = float(np.max([abs(ref[k]) for k in ("U0", "K0", "U1", "K1")]))   # (NaN with a negative prior sigma)
    if case.L == 0:   # q does not move: the gradient reaches only K1
        d, dr = res["K1"] - res["K0"], ref["K1"] - ref["K0"]
        out["K1-K0"] = (np.array([d]), np.array([dr]), abs(dr), F32_EPS * max(abs(ref["K0"]), abs(ref["K1"])))
    else:
        g, gr = gradient_move(res, case), gradient_move(ref, case)
        qmax = float(np.abs(np.asarray(ref["q_proposed"], dtype=np.float64)).max())
        whole = float(np.abs(gr).max())
        for name, sl in blocks(case.spec):
            out[f"move {name}"] = (g[sl], gr[sl], max(float(np.abs(gr[sl]).max()), 1e-3 * whole), F32_EPS * qmax)
    for k in SCALARS:
        scale = energy if k == "log_ratio" else abs(ref[k])
        floor = F32_EPS * (energy if k == "log_ratio" else abs(ref[k]))
        out[k] = (np.array([res[k]]), np.array([ref[k]]), scale, floor)
    return out


def _err(v, r):
    v, r = np.asarray(v, dtype=np.float64), np.asarray(r, dtype=np.float64)
    both_nan = np.isnan(v) & np.isnan(r)     # a negative prior sigma: NaN potential on both sides
    d = np.abs(np.where(both_nan, 0.0, v - r))
    return float(np.where(np.isnan(d), np.inf, d).max())


@functools.lru_cache(maxsize=None)
def _tolerances(name: str):
    case = CASE_BY_NAME[name]
    data = case_data(case)
    return measured_rel32(case, [(oracle_result(case, data, c, np.float32), oracle_result(case, data, c, np.float64))
                                 for c in check_chains(case.P)])


def tolerances(case: HmcCase):
    """{quantity: the float32 oracle's largest difference from the float64 one over the checked chains, relative to the
    quantity's scale}.  `compare` allows FACTOR times that, not below the float32 rounding of what is stored and never
    above CAP of the scale."""
    return dict(_tolerances(case.name))


def measured_rel32(case: HmcCase, pairs):
    """The rule of `tolerances` on other inputs than the case's own (a later proposal of a sequence): `pairs` are the
    (float32 oracle, float64 oracle) results of the chains compared."""
    rel = {}
    for f32, ref in pairs:
        for k, (v, r, scale, _) in quantities(f32, ref, case).items():
            e = _err(v, r) / scale if scale > 0 and np.isfinite(scale) else 0.0
            rel[k] = max(rel.get(k, 0.0), e)
    return rel


@functools.lru_cache(maxsize=None)
def _sequence_rel32(name: str, n: int):
    case = CASE_BY_NAME[name]
    data = case_data(case)
    rel = tolerances(case)
    q = data.q0.astype(np.float64)
    for k in range(n):
        pairs = []
        for c in range(case.P):
            z = philox_z(case, c, step=case.step + k)
            ref = oracle_result(case, data, c, np.float64, u=0.0 if k == 2 else 2.0, q=q[c].astype(np.float32), z=z)
            pairs.append((oracle_result(case, data, c, np.float32, u=0.0 if k == 2 else 2.0, q=q[c].astype(np.float32), z=z), ref))
            q[c] = ref["q_proposed"] if k != 2 else q[c]
        for key, v in measured_rel32(case, pairs).items():
            rel[key] = max(rel[key], v)
    return rel


def sequence_rel32(case: HmcCase, n: int):
    """The float32 oracle's largest differences over a sequence of n Philox proposals carried forward by the float64
    oracle itself (the third rejected), and over the case's own inputs: every proposal has new inputs, and one float32
    run per quantity is a single draw of the reference's error (a K1 that happens to round well gives 1e-8 where the
    next gives 1e-7), so the sequence test takes the largest of its 1 + n measurements.  Computed on the CPU alone."""
    return dict(_sequence_rel32(case.name, n))


def compare(result, ref, case: HmcCase, what: str = "", rel32=None):
    """`result` against the float64 oracle's `ref` for one chain (both from `result_from`).  Raises AssertionError with
    the quantity that missed; returns {quantity: (error, tolerance)}.  `rel32`: the float32 oracle's differences where
    the inputs are not the case's own (`sequence_rel32`)."""
    rel32 = tolerances(case) if rel32 is None else rel32
    report = {}
    for k, (v, r, scale, floor) in quantities(result, ref, case).items():
        assert np.all(np.isfinite(v) | np.isnan(r)), f"{what}{case.name}: {k}: non-finite where the oracle is finite"
        if not np.isfinite(scale):
            assert _err(v, r) == 0.0, f"{what}{case.name}: {k}: {v} where the oracle has {r}"
            continue
        tol = min(max(FACTOR * rel32[k] * scale, floor), CAP * scale)
        err = _err(v, r)
        report[k] = (err, tol)
        assert err <= tol, (f"{what}{case.name}: {k}: error {err:.3e} > tolerance {tol:.3e} (scale {scale:.3e}, float32 oracle "
                            f"{rel32[k]:.2e} of the scale, floor {floor:.2e})")
    assert result["accepted"] == ref["accepted"], f"{what}{case.name}: accepted {result['accepted']}, oracle {ref['accepted']}"
    q, q0, qp = (np.asarray(result[k], dtype=np.float32) for k in ("q", "q0", "q_proposed"))
    if result["accepted"]:
        assert np.array_equal(q, qp), f"{what}{case.name}: the accepted q is not the proposal of the burning call"
    else:
        assert np.array_equal(q.view(np.uint32), q0.view(np.uint32)), f"{what}{case.name}: a rejected q is not restored bit for bit"
    return report
