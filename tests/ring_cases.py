"""The case table of k_dense_fwd_ring (csrc/pyz_gemm_ring.h) and the launch rules it relies on (a plain module: imported
by the ring tests, in the style of dense_cases.py).

The ring kernel is the first one tried for every forward layer.  This module restates in plain Python, each with its
source location, when a launch takes it (`ring_variant`), which instantiation runs (`ring_sub`, `ring_expr`), the slab
arithmetic of a workgroup (`ring_ks`, `ring_ns`, `ring_mis`, `copy_slabs`) and the numbers `PyzRingGeom` derives for an
instantiation (`geom`); names the cells of the coverage table (`CELLS`, `reached_cells`) and lists the smallest cases that
together reach every cell.  tests/test_ring_dispatch_table.py pins the restatement to the source on the CPU;
tests/test_gpu_ring_matrix.py runs the cases against the float64 oracle."""

from __future__ import annotations

from typing import NamedTuple

import dense_cases as dc
from dense_cases import cdiv
from oracle import mlp as o_mlp

# ---------------------------------------------------------------- launch rules (csrc/pyz_gemm_ring.h)
RING_MINWG, RING_MAXWG = 192, 1024   # pyz_fwd_ring_variant: PYZ_FWD_RING_MINWG / _MAXWG (read once per process: left alone)
RING_N = (192, 200)                  # pyz_fwd_ring_variant: g.N > 192 && g.N <= 200
RING_CGRP = 200                      # pyz_fwd_ring_variant: column groups of 200 (PYZ_FWD_RING_WIDE, opt-in)
RING_WIDE_MAX_N = 1600
NL, NCT = 204, 13                    # pyz_launch_fwd_ring: the one image width / sub-tile count that is instantiated
BK, NBUF = 16, 4                     # PyzRingGeom
INSTANCES = ((2, 4), (1, 4), (2, 8), (1, 8))   # pyz_launch_fwd_ring: (SUB, NW) in the order of its if-chain
HOST_CUS = 256                       # the CU count the host test assumes (the GPU test reads the device's)
ENV_ONCE = ("PYZ_FWD_RING", "PYZ_FWD_RING_MINWG", "PYZ_FWD_RING_MAXWG", "PYZ_FWD_RING_SUB", "PYZ_FWD_RING_WAVES")
ENV_FORBIDDEN = ENV_ONCE + ("PYZ_FWD_RING_WIDE",) + dc.ENV_FORBIDDEN   # the expected launches assume their defaults


def ring_wgs(grid_batch: int, P: int, N: int) -> int:
    """pyz_fwd_ring_variant / pyz_launch_fwd_ring: 32-row blocks x particles x column groups."""
    n_cg = cdiv(N, RING_CGRP) if N > RING_CGRP else 1
    return cdiv(grid_batch, 32) * P * n_cg


def ring_variant(K, N, grid_batch, P, lda, in_pstride, w_off, in_addr=0, theta_addr=0, gather_addr=None, wide=0, on=1,
                 min_wg=RING_MINWG, max_wg=RING_MAXWG) -> int:
    """pyz_fwd_ring_variant in full.  in_addr / theta_addr / gather_addr: the byte addresses of g.in, g.theta and
    g.gather_out (None: no batch copy); only their low bits matter."""
    if not on:
        return 0
    wgs = ring_wgs(grid_batch, P, N)
    if wgs < min_wg or wgs > max_wg:
        return 0
    if K % 4 or N % 4 or lda % 4 or w_off % 4 or (P > 1 and in_pstride % 4):
        return 0
    if (in_addr & 15) or (gather_addr is not None and (gather_addr & 15)):
        return 0
    if theta_addr & 3:
        return 0
    if RING_N[0] < N <= RING_N[1]:
        return 1
    if N > RING_CGRP and N % RING_CGRP == 0 and N <= RING_WIDE_MAX_N and wide:
        return 1
    return 0


def ring_sub(wgs: int, cus: int = HOST_CUS, sub_env: int = 0) -> int:
    """pyz_launch_fwd_ring: two sub-slabs per ring slot while the launch has no second workgroup per CU anyway."""
    return sub_env if sub_env else (2 if 4 * wgs <= 5 * cus else 1)


def ring_expr(sub: int, nw: int = 8) -> str:
    """The kernel expression KernelProbe reports for pyz_launch_fwd_ring's launch."""
    return f"k_dense_fwd_ring<{NL}, {NCT}, {sub}, {nw}>"


def ring_ks(sub: int) -> int:          # PyzRingGeom: KS = BK * SUB
    return BK * sub


def ring_ns(K: int, sub: int) -> int:  # k_dense_fwd_ring: ns_all = (K + KS - 1) / KS
    return cdiv(K, ring_ks(sub))


def ring_mis(p: int, D: int, w_off: int) -> int:
    """k_dense_fwd_ring: floats between the 16-byte aligned base and W[0][0] of particle p (theta itself 16-byte aligned:
    a fresh device allocation)."""
    return (p * D + w_off) % 4


def copy_slabs(p: int, P: int, ns: int) -> list:
    """k_dense_fwd_ring, sync_point: the slabs whose A block workgroup (p, rows) stores to the batch copy (s % P == p)."""
    return [s for s in range(ns) if s % P == p]


def b_rows_past_k(K: int, sub: int) -> int:
    """Rows k >= K of [W; b] that the last slab's B image covers."""
    return ring_ns(K, sub) * ring_ks(sub) - K


class Geom(NamedTuple):
    KS: int
    PR: int
    B_INSTR: int
    NI1: int
    NI: int
    A_OFF: int
    SUBSLOT: int
    SLOT: int
    LDS_BYTES: int
    CT: int
    T: int
    IPW: int


def geom(sub: int, nw: int, nl: int = NL, nct: int = NCT) -> Geom:
    """PyzRingGeom<NL, NCT, SUB, NW> (and IPW of k_dense_fwd_ring)."""
    PR = nl // 4
    B_INSTR = (BK * PR + 63) // 64
    NI1 = B_INSTR + 2
    NI = sub * NI1
    A_OFF = B_INSTR * 1024
    SUBSLOT = A_OFF + 2048
    SLOT = sub * SUBSLOT
    return Geom(BK * sub, PR, B_INSTR, NI1, NI, A_OFF, SUBSLOT, SLOT, NBUF * SLOT + 1024, (nct + 1) // 2, 4 * sub, (NI + 3) // 4)


def geom_asserts(g: Geom, nw: int, nl: int = NL, nct: int = NCT) -> dict:
    """The static_asserts of PyzRingGeom, by their message."""
    return {"waves per workgroup": nw in (4, 8),
            "every moving wave issues DMA instructions": g.NI >= 4,
            "LDS of a CU": g.LDS_BYTES <= 160 * 1024,
            "the wait counts assume two slabs in flight behind the one awaited": NBUF == 4,
            "row stride of the B image: the four reduction quarters on disjoint banks": nl % 8 == 4,
            "column sub-tiles": 2 <= nct <= 14 and 16 * nct <= nl + 12}


# ---------------------------------------------------------------- cases
class RingCase(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    loss: str
    P: int = 64
    batch: int = 96
    gathered: bool = False   # x has more rows than the batch; the batch comes through row_idx
    x_offset: bool = False   # x starts 4 bytes into its storage
    env: dict = {}           # PYZ_FWD_LDS_MINWG (read per call)
    isolate: bool = False    # also run with every odd particle's parameters non-finite
    negative: str = ""       # why no layer of the case may take the ring ("" = layer `ring_layer` must)

    @property
    def spec(self) -> o_mlp.MLPSpec:
        return o_mlp.MLPSpec(self.dims, self.acts, self.loss)

    @property
    def max_batch(self) -> int:
        return self.batch + 3

    @property
    def dense(self) -> dc.DenseCase:
        """The same case for dense_cases.case_data / batch_rows (edge-weighted data, unit-rms pre-activations)."""
        return dc.DenseCase(self.name, self.dims, self.acts, self.loss, self.P, self.batch, self.gathered, self.x_offset,
                            dict(self.env), False, 0)

    @property
    def ring_layer(self) -> int:
        """The layer the case is about: the one 192 .. 204 units wide (every case has exactly one)."""
        (l,) = [l for l, N in enumerate(self.dims[1:]) if 192 <= N <= 204]
        return l


class FwdLaunch(NamedTuple):
    layer: int
    kernel: str     # expression KernelProbe reports
    K: int
    N: int
    sub: int        # 0: not the ring
    copy: bool      # leaves the batch copy


def fwd_launches(case: RingCase, call: str = "forward", cus: int = HOST_CUS, sub_env: int = 0, nw: int = 8) -> list:
    """The forward launches of `forward` / `predict` (call = "forward": every layer) or `loss_grad` (call = "grad": the
    hidden layers of these fused models), restating pyz_api.hip forward_args / launch_forward / launch_loss_backward."""
    dims, P, B, D = case.dims, case.P, case.batch, case.spec.n_params
    L = len(dims) - 1
    assert dc.can_fuse(dims), "every ring case ends in a layer the head kernel takes"
    grad = call == "grad"
    offs = dc.w_offsets(dims)
    out = []
    for l in range(L - 1 if grad else L):
        K, N = dims[l], dims[l + 1]
        aligned = not (l == 0 and case.x_offset)
        in_pstride = 0 if l == 0 else case.max_batch * K            # forward_args: (long long)m->max_batch * g.K
        copy = grad and case.gathered and L > 1 and l == 0           # launch_loss_backward: xb; forward_args: layer 0 only
        v = ring_variant(K, N, B, P, K, in_pstride, offs[l], in_addr=0 if aligned else 4, gather_addr=0 if copy else None)
        if v:
            sub = ring_sub(ring_wgs(B, P, N), cus, sub_env)
            out.append(FwdLaunch(l, ring_expr(sub, nw), K, N, sub, copy))
            continue
        S, _ = dc.pick_waves(dc.fwd_tiles(B, N) * P, dc.fwd_steps(K))
        lds = dc.fwd_takes_lds(K, N, B, P, D, offs[l], S, aligned, 1, int(case.env.get("PYZ_FWD_LDS_MINWG", dc.LDS_MINWG)))
        out.append(FwdLaunch(l, f"k_dense_fwd_lds<{dc.lds_nt(N)}>" if lds else "k_dense_fwd", K, N, 0, copy))
    return out


def ring_launch(case: RingCase, call: str = "forward", cus: int = HOST_CUS, sub_env: int = 0):
    """The ring launch of a positive case (None when the call does not reach the ring layer)."""
    got = [f for f in fwd_launches(case, call, cus, sub_env) if f.sub]
    assert len(got) <= 1
    return got[0] if got else None


def crosses_particles(case: RingCase, sub: int) -> bool:
    """Does the last slab's B image, taken to the end of its rows k >= K, run past this particle's parameters?  (What
    the kernel read before its buffer range ended at &W[K][0].)"""
    l = case.ring_layer
    K, N = case.dims[l], case.dims[l + 1]
    own = case.spec.n_params - dc.w_offsets(case.dims)[l] - K * N     # the particle's floats behind this layer's W
    return b_rows_past_k(K, sub) * N > own


# ---------------------------------------------------------------- the coverage table
ISSUE_K = (4, 16, 20, 36, 48, 64, 68, 80, 132)
NS_CELLS = ("1", "2", "3", "4", "5", ">=6")
REM_CELLS = {1: (0, 4, 12), 2: (0, 4, 12, 16, 20)}
NEGATIVES = ("N=192", "N=204", "K%4=2", "x offset", "wgs=191")
ACTS = ("relu", "tanh", "sigmoid", "linear")
CELLS = frozenset(
    [f"N={N}" for N in (196, 200)] +
    [f"SUB={s} ns={n}" for s in (1, 2) for n in NS_CELLS] +
    [f"SUB={s} K%KS={r}" for s in (1, 2) for r in REM_CELLS[s]] +
    [f"K={K}" for K in ISSUE_K] +
    [f"mis D%4={r}" for r in range(4)] +
    ["rows contiguous"] + [f"rows gathered batch%32={r}" for r in (0, 1, 31)] + ["rows one live row in the last block"] +
    ["copy P>ns", "copy P<ns", "hidden layer, per-particle input"] +
    [f"act {a}" for a in ACTS] +
    ["isolation K%KS!=0 crossing", "isolation K%KS==0"] +
    [f"negative {n}" for n in NEGATIVES] + ["negative runs k_dense_fwd", "negative runs k_dense_fwd_lds",
                                            "isolation k_dense_fwd", "isolation k_dense_fwd_lds"])


def reached_cells(case: RingCase, cus: int = HOST_CUS) -> set:
    """The cells a case reaches under the default variant rule on `cus` compute units."""
    cells = set()
    if case.negative:
        fl = fwd_launches(case, "forward", cus)
        assert not any(f.sub for f in fl) and not any(f.sub for f in fwd_launches(case, "grad", cus)), case.name
        cells.add(f"negative {case.negative}")
        kern = fl[case.ring_layer].kernel.split("<")[0]
        cells.add(f"negative runs {kern}")
        if case.isolate:
            cells.add(f"isolation {kern}")
        return cells & CELLS
    f = ring_launch(case, "forward", cus)
    assert f is not None, f"{case.name}: no layer takes the ring"
    K, N, sub, P, B, D = f.K, f.N, f.sub, case.P, case.batch, case.spec.n_params
    ns, rem = ring_ns(K, sub), K % ring_ks(sub)
    cells.add(f"N={N}")
    cells.add(f"SUB={sub} ns={ns if ns < 6 else '>=6'}")
    cells.add(f"SUB={sub} K%KS={rem}")
    cells.add(f"K={K}")
    if P >= 4 and {ring_mis(p, D, dc.w_offsets(case.dims)[f.layer]) for p in range(P)} == ({0, 1, 2, 3} if D % 2 else
                                                                                          {0, 2} if D % 4 else {0}):
        cells.add(f"mis D%4={D % 4}")
    if f.layer == 0:
        cells.add(f"rows gathered batch%32={B % 32}" if case.gathered else "rows contiguous")
    else:
        cells.add("hidden layer, per-particle input")
    if B % 32 == 1:
        cells.add("rows one live row in the last block")
    g = ring_launch(case, "grad", cus)
    if g is not None and g.copy:
        cells.add("copy P>ns" if P > ns else "copy P<ns" if P < ns else "copy P==ns")
    cells.add(f"act {case.acts[f.layer]}")
    if case.isolate:
        if rem == 0:
            cells.add("isolation K%KS==0")
        elif crosses_particles(case, sub):
            cells.add("isolation K%KS!=0 crossing")
    return cells & CELLS


def _c(name, dims, acts, loss, P=64, batch=96, gathered=False, x_offset=False, env=None, isolate=False, negative=""):
    return RingCase(name, tuple(dims), tuple(acts), loss, P, batch, gathered, x_offset, dict(env or {}), isolate, negative)


SC, MS = dc.SC, dc.MS
R, T, G, LN, SM = dc.R, dc.T, dc.G, dc.LN, dc.SM

CASES = [
    # ---- SUB = 2 by the default rule (64 particles x 3 .. 5 row blocks: at most 320 workgroups on 256 CUs), KS = 32:
    # one case per slab count; the remainders 16 and 20 leave a whole second sub-slab past K
    _c("s2_k16_ns1_n196", (16, 196, 5), (T, SM), SC, batch=96, gathered=True),
    _c("s2_k20_ns1_iso", (20, 200, 3), (G, SM), SC, batch=97, gathered=True, isolate=True),
    _c("s2_k44_ns2_rem12", (44, 200, 2), (LN, LN), MS, batch=127, gathered=True),
    _c("s2_k64_ns2_rem0_iso", (64, 200, 3), (R, SM), SC, batch=96, isolate=True),
    _c("s2_k68_ns3", (68, 196, 4), (T, SM), SC, batch=128),
    _c("s2_k100_ns4", (100, 200, 5), (R, SM), SC, batch=160, gathered=True),
    _c("s2_k132_ns5_p4_copy", (132, 200, 4), (R, SM), SC, P=4, batch=1537, gathered=True),
    _c("s2_k164_ns6", (164, 200, 6), (G, G), MS, batch=99),
    _c("s2_hidden_k36", (12, 36, 200, 2), (T, R, LN), MS, batch=96, gathered=True),
    # ---- SUB = 1 (64 particles x 6 row blocks = 384 workgroups), KS = 16; batch 161 is the block with one live row
    _c("s1_k4_ns1", (4, 200, 4), (R, SM), SC, batch=161),
    _c("s1_k20_ns2_iso", (20, 200, 3), (LN, SM), SC, batch=161, gathered=True, isolate=True),
    _c("s1_k48_ns3", (48, 196, 7), (G, SM), SC, batch=191, gathered=True),
    _c("s1_k64_ns4", (64, 200, 2), (T, T), MS, batch=192, gathered=True),
    _c("s1_k80_ns5", (80, 200, 5), (R, SM), SC, batch=161),
    _c("s1_k108_ns7_rem12", (108, 196, 3), (T, SM), SC, batch=170),
    # ---- launches the ring must refuse: the kernel that runs instead, against the same oracle
    _c("neg_n192", (20, 192, 3), (R, SM), SC, batch=96, isolate=True, negative="N=192"),
    _c("neg_n204_lds", (20, 204, 4), (T, SM), SC, batch=161, env=dc.LDS_ANY, isolate=True, negative="N=204"),
    _c("neg_k18", (18, 200, 3), (G, SM), SC, batch=96, negative="K%4=2"),
    _c("neg_x_offset", (20, 200, 3), (R, SM), SC, batch=96, x_offset=True, negative="x offset"),
    _c("neg_wgs191", (20, 200, 3), (T, SM), SC, P=1, batch=6100, negative="wgs=191"),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), "case names must be unique"
POSITIVE = [c for c in CASES if not c.negative]
ISOLATION = [c for c in CASES if c.isolate]

# the forced variants (the switches are read once per process: a child process per line): (name, environment, SUB, waves).
# With eight waves "the opposite of the default" is SUB = 1 for the s2_* cases and SUB = 2 for the s1_* cases: one child
# each, both run every positive case.
FORCED = [("waves4_sub1", {"PYZ_FWD_RING_WAVES": "4", "PYZ_FWD_RING_SUB": "1"}, 1, 4),
          ("waves4_sub2", {"PYZ_FWD_RING_WAVES": "4", "PYZ_FWD_RING_SUB": "2"}, 2, 4),
          ("waves8_sub1", {"PYZ_FWD_RING_SUB": "1"}, 1, 8),
          ("waves8_sub2", {"PYZ_FWD_RING_SUB": "2"}, 2, 8)]


def case_data(case: RingCase):
    return dc.case_data(case.dense)


def batch_rows(case: RingCase, x, y, idx):
    return dc.batch_rows(case.dense, x, y, idx)
