"""The ring case table (tests/ring_cases.py) against the library's source, on the CPU.

The launch rule of k_dense_fwd_ring, the rule that picks its instantiation, the slab arithmetic of a workgroup and the
numbers PyzRingGeom derives are read out of pyz_gemm_ring.h / pyz_api.hip and compared with the plain-Python
restatement; the cells the cases reach are compared with the coverage table, and every case must be the only one that
reaches some cell, so deleting a case or moving a threshold fails here with the name of the lost cell."""

import os
import re

import numpy as np
import pytest

import dense_cases as dc
import ring_cases as rc
from ring_cases import CASES, CELLS, FORCED, ISOLATION, POSITIVE, fwd_launches, reached_cells, ring_variant

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesian_inference_for_nn_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def function_body(text, head):
    i = text.index(head)
    return text[i:text.index("\n}", i)]


RING, API = src("pyz_gemm_ring.h"), src("pyz_api.hip")


# ---------------------------------------------------------------- the restatement against the source
def test_switches_and_their_defaults():
    for name, default in (("PYZ_FWD_RING", 1), ("PYZ_FWD_RING_MINWG", rc.RING_MINWG), ("PYZ_FWD_RING_MAXWG", rc.RING_MAXWG),
                          ("PYZ_FWD_RING_SUB", 0), ("PYZ_FWD_RING_WAVES", 8)):
        assert re.findall(r'static const int \w+ = pyz_env_int\("%s", (-?\d+)\)' % name, RING) + \
            re.findall(r', \w+ = pyz_env_int\("%s", (-?\d+)\)' % name, RING) == [str(default)], name
        assert name in rc.ENV_ONCE          # read once per process: the GPU module refuses to run with them set
    assert 'pyz_env_int("PYZ_FWD_RING_WIDE", 0)' in RING and "PYZ_FWD_RING_WIDE" in rc.ENV_FORBIDDEN
    assert (rc.RING_MINWG, rc.RING_MAXWG, rc.RING_N) == (dc.RING_MINWG, dc.RING_MAXWG, dc.RING_N)


def test_launch_rule_matches_the_source_line_by_line():
    rv = function_body(RING, "static inline int pyz_fwd_ring_variant(")
    lines = [l.strip() for l in rv.splitlines() if l.strip() and not l.strip().startswith("//")]
    assert lines[1:] == [
        'static const int on = pyz_env_int("PYZ_FWD_RING", 1);',
        'static const int min_wg = pyz_env_int("PYZ_FWD_RING_MINWG", 192);',
        'static const int max_wg = pyz_env_int("PYZ_FWD_RING_MAXWG", 1024);',
        "if (!on) return 0;",
        "const int n_cg = g.N > 200 ? (g.N + 199) / 200 : 1;      // column groups of 200",
        "const long long wgs = (long long)((grid_batch + 31) / 32) * P * n_cg;",
        "if (wgs < min_wg || wgs > max_wg) return 0;",
        "if (g.K % 4 || g.N % 4 || g.lda % 4 || g.w_off % 4 || (P > 1 && g.in_pstride % 4)) return 0;",
        "if ((reinterpret_cast<uintptr_t>(g.in) & 15) || (g.gather_out && (reinterpret_cast<uintptr_t>(g.gather_out) & 15))) return 0;",
        "if ((reinterpret_cast<uintptr_t>(g.theta) & 3)) return 0;",
        "if (g.N > 192 && g.N <= 200) return 1;   // <204, 13>",
        "if (g.N > 200 && g.N % 200 == 0 && g.N <= 1600 && pyz_env_int(\"PYZ_FWD_RING_WIDE\", 0)) return 1;",
        "return 0;"], lines
    assert (rc.RING_CGRP, rc.RING_WIDE_MAX_N) == (200, 1600)
    # what forward_args hands the rule (pyz_api.hip)
    fa = function_body(API, "DenseArgs forward_args(")
    for text in ("g.in_pstride = 0;", "g.gather_out = row_idx ? gather_out : nullptr;", "g.in_pstride = (long long)m->max_batch * g.K;",
                 "g.lda = g.K;", "g.w_off = m->w_off[l];"):
        assert text in fa, text
    assert "if (pyz_launch_fwd_ring(g, grid_batch, P, st)) continue;" in function_body(API, "void launch_forward(")
    assert "launch_forward(m, theta, theta_ps, P, x, row_idx, grid_batch, ctl, st, xb, m->L - 1);" in API


def test_launch_rule_at_its_edges():
    take = lambda **kw: ring_variant(**{**dict(K=20, N=200, grid_batch=96, P=64, lda=20, in_pstride=0, w_off=0), **kw})
    assert take() == 1
    assert [take(N=N) for N in (188, 192, 196, 200, 204, 198)] == [0, 0, 1, 1, 0, 0]
    assert [take(grid_batch=b) for b in (64, 65, 512, 513)] == [0, 1, 1, 0]          # 128, 192, 1024, 1088 workgroups
    assert take(P=1, grid_batch=191 * 32) == 0 and take(P=1, grid_batch=191 * 32 + 1) == 1
    assert take(K=18, lda=18) == 0 and take(lda=22) == 0 and take(w_off=2) == 0
    assert take(in_pstride=99 * 18) == 0 and take(in_pstride=99 * 18, P=1, grid_batch=6144) == 1
    assert take(in_addr=4) == 0 and take(in_addr=16) == 1
    assert take(gather_addr=8) == 0 and take(gather_addr=32) == 1
    assert take(theta_addr=2) == 0 and take(theta_addr=4) == 1     # a particle's block needs no more than 4 bytes
    assert take(on=0) == 0 and take(min_wg=193) == 0
    assert take(N=400) == 0 and take(N=400, wide=1, grid_batch=48) == 1 and take(N=1800, wide=1, grid_batch=16) == 0
    # dense_cases' shorter rule agrees wherever its terms are the only ones in play
    for K, N, B, P in ((784, 200, 1024, 8), (20, 196, 96, 64), (18, 200, 96, 64), (20, 204, 96, 64), (20, 200, 32, 5)):
        assert dc.fwd_ring_variant(K, N, B, P, 0, True) == ring_variant(K, N, B, P, K, 0, 0)


def test_variant_rule_matches_the_source():
    body = function_body(RING, "static inline bool pyz_launch_fwd_ring(")
    assert "const int sub = sub_env ? sub_env : (4 * wgs <= 5 * (long long)pyz_cu_count() ? 2 : 1);" in body
    assert "const long long wgs = (long long)((grid_batch + 31) / 32) * P * (g.N > 200 ? (g.N + 199) / 200 : 1);" in body
    chain = re.findall(r"(if \(nw == 4 && sub == 2\)|else if \(nw == 4\)|else if \(sub == 2\)|else) PYZ_LAUNCH_FWD_RING_AS\((\d), (\d)\);", body)
    assert [(int(s), int(w)) for _, s, w in chain] == list(rc.INSTANCES), chain
    assert [c for c, _, _ in chain] == ["if (nw == 4 && sub == 2)", "else if (nw == 4)", "else if (sub == 2)", "else"]
    # the probe reports the expression as written at the launch: the instantiation must be spelled out there
    assert "PYZ_LAUNCH((k_dense_fwd_ring<204, 13, SUB, NW>), dim3((unsigned)((wgs_ + 7) / 8 * 8)), dim3(64 * NW), 0, st, a);" in RING
    assert rc.ring_expr(2) == "k_dense_fwd_ring<204, 13, 2, 8>" and rc.ring_expr(1, 4) == "k_dense_fwd_ring<204, 13, 1, 4>"
    assert "PYZ_LAUNCH((k_dense_fwd_ring<204, 13, 1, 8>)," in function_body(RING, "static inline void pyz_launch_fwd_ring_ksplit(")
    assert [rc.ring_sub(w) for w in (192, 320, 321, 1024)] == [2, 2, 1, 1]           # 256 CUs
    assert [rc.ring_sub(w, cus=304) for w in (380, 381)] == [2, 1]
    assert rc.ring_sub(192, sub_env=1) == 1 and rc.ring_sub(1024, sub_env=2) == 2
    assert [(n, s, w) for n, _, s, w in FORCED] == [("waves4_sub1", 1, 4), ("waves4_sub2", 2, 4), ("waves8_sub1", 1, 8),
                                                   ("waves8_sub2", 2, 8)]
    for _, env, s, w in FORCED:
        assert env == {**({"PYZ_FWD_RING_WAVES": "4"} if w == 4 else {}), "PYZ_FWD_RING_SUB": str(s)} and set(env) <= set(rc.ENV_ONCE)


def test_slab_arithmetic_matches_the_source():
    k = function_body(RING, "__global__ void __launch_bounds__(64 * NW) k_dense_fwd_ring(")
    for text in ("const int ns_all = (K + KS - 1) / KS;",
                 "const float *wl = g.theta + (long long)p * g.theta_pstride + g.w_off;",
                 "const int mis = (int)((reinterpret_cast<uintptr_t>(wl) & 15u) >> 2);",
                 "const long long b_bytes = ((long long)K * N + mis) * 4;",      # the B image ends at &W[K][0] of this particle
                 "if (copies && (s % P) == p) {",
                 "const float *src = (KS * (s_lo + s) + koffA[u] < K) ? srcA[u] : pyz_zero16;",
                 "bias[ct] = wl[(long long)K * N + min(col0 + col, N - 1)];",
                 "if (mm < batch && col < g.cgrp_w && col0 + col < N) {",
                 "if (1 < ns) issue(1);", "if (2 < ns) issue(2);", "wait_own(min(2, ns - 1));",
                 "if (moves && s + NBUF - 1 < ns) issue(s + NBUF - 1);"):
        assert text in k, text
    assert [rc.ring_ks(s) for s in (1, 2)] == [16, 32]
    assert [rc.ring_ns(K, 1) for K in rc.ISSUE_K] == [1, 1, 2, 3, 3, 4, 5, 5, 9]
    assert [rc.ring_ns(K, 2) for K in rc.ISSUE_K] == [1, 1, 1, 2, 2, 2, 3, 3, 5]
    assert [rc.ring_ns(K, 2) for K in (100, 164)] == [4, 6] and rc.ring_ns(784, 2) == 25 and rc.ring_ns(784, 1) == 49
    assert [rc.ring_mis(p, 4803, 0) for p in range(5)] == [0, 3, 2, 1, 0] and [rc.ring_mis(p, 159010, 0) for p in range(3)] == [0, 2, 0]
    assert rc.ring_mis(1, 8270, 468) == 2
    assert rc.copy_slabs(0, 4, 5) == [0, 4] and rc.copy_slabs(3, 4, 5) == [3] and rc.copy_slabs(5, 64, 2) == []
    # the issue's example: 784 -> 200 -> 10 with SUB = 2 covers rows 784 .. 799, 3 200 floats, 990 of them the next particle's
    assert rc.b_rows_past_k(784, 2) * 200 == 3200 and 3200 - (200 + 201 * 10) == 990
    assert rc.b_rows_past_k(20, 2) * 200 == 2400 and 4803 - 20 * 200 == 803


def test_geometry_of_the_four_instantiations():
    g_text = function_body(RING, "struct PyzRingGeom {")
    for text in ("static constexpr int BK = 16, NBUF = 4;", "static constexpr int KS = BK * SUB;", "static constexpr int PR = NL / 4;",
                 "static constexpr int B_INSTR = (BK * PR + 63) / 64;", "static constexpr int NI1 = B_INSTR + 2;",
                 "static constexpr int NI = SUB * NI1;", "static constexpr int A_OFF = B_INSTR * 1024;",
                 "static constexpr int SUBSLOT = A_OFF + 2048;", "static constexpr int SLOT = SUB * SUBSLOT;",
                 "static constexpr int LDS_BYTES = NBUF * SLOT + 1024;", "static constexpr int CT = (NCT + 1) / 2;",
                 "static constexpr int T = 4 * SUB;"):
        assert text in g_text, text
    assert "constexpr int IPW = (NI + 3) / 4;" in RING
    messages = re.findall(r'static_assert\(.*, "([^"]+)"\);', g_text)
    for sub, nw in rc.INSTANCES:
        g = rc.geom(sub, nw)
        checks = rc.geom_asserts(g, nw)
        assert sorted(checks) == sorted(messages)
        assert all(checks.values()), (sub, nw, checks)
        assert (g.PR, g.B_INSTR, g.NI1, g.A_OFF, g.SUBSLOT, g.CT) == (51, 13, 15, 13312, 15360, 7)
        assert (g.KS, g.NI, g.SLOT, g.LDS_BYTES, g.T, g.IPW) == ((16, 15, 15360, 62464, 4, 4) if sub == 1 else
                                                                 (32, 30, 30720, 123904, 8, 8))
        assert 16 * g.PR >= 16 * 51 and 64 * g.B_INSTR >= 16 * g.PR        # the DMA instructions cover the 16 x 51 pieces
    assert not rc.geom_asserts(rc.geom(1, 8, nl=208), 8, nl=208)["row stride of the B image: the four reduction quarters on disjoint banks"]
    assert not rc.geom_asserts(rc.geom(4, 8), 8)["LDS of a CU"]


# ---------------------------------------------------------------- the cases against the table
def test_cases_reach_every_cell_and_each_case_is_needed():
    by_cell = {}
    for c in CASES:
        for cell in reached_cells(c):
            by_cell.setdefault(cell, []).append(c.name)
    lost = sorted(CELLS - set(by_cell))
    assert not lost, f"cells no case reaches: {lost}"
    assert set(by_cell) == set(CELLS)
    for c in CASES:
        only = [cell for cell, names in by_cell.items() if names == [c.name]]
        assert only, f"dropping {c.name} loses no cell"


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_cell_is_reached(cell):
    assert any(cell in reached_cells(c) for c in CASES), f"no case reaches the cell '{cell}'"


def test_table_has_the_cells_the_issue_lists():
    assert len(CELLS) == 2 + 12 + 8 + 9 + 4 + 5 + 3 + 4 + 2 + 5 + 4 and len(CASES) == 20 and len(POSITIVE) == 15
    assert rc.ISSUE_K == (4, 16, 20, 36, 48, 64, 68, 80, 132) and rc.NEGATIVES == ("N=192", "N=204", "K%4=2", "x offset", "wgs=191")


def test_expected_launches_and_sizes():
    for c in CASES:
        wgs = rc.ring_wgs(c.batch, c.P, c.dims[c.ring_layer + 1])
        fl, gl = fwd_launches(c), fwd_launches(c, "grad")
        assert len(fl) == len(c.dims) - 1 and len(gl) == len(c.dims) - 2
        assert c.P * c.max_batch * max(c.dims) <= 4 * 1024 * 1024 and c.spec.n_params * c.P * 4 < 2 ** 31, c.name
        assert not c.env or (c.negative and set(c.env) == {"PYZ_FWD_LDS_MINWG"}), c.name
        if c.negative:
            assert not any(f.sub for f in fl + gl), c.name
            assert (wgs == 191) == (c.negative == "wgs=191") and (wgs >= 192 or c.negative == "wgs=191"), c.name
            continue
        assert rc.RING_MINWG <= wgs <= rc.RING_MAXWG, c.name
        ring = [f for f in fl if f.sub]
        assert [f.layer for f in ring] == [c.ring_layer] and [f.layer for f in gl if f.sub] == [c.ring_layer], c.name
        assert ring[0].sub == int(c.name[1]) and ring[0].kernel == rc.ring_expr(ring[0].sub), c.name      # s1_* / s2_* by the default rule
        assert all(f.kernel == "k_dense_fwd" for f in fl if not f.sub), c.name
        for cus in (256, 304):     # whatever the device: the forced children still meet both SUB
            assert {rc.ring_launch(c, "forward", cus, s).sub for s in (1, 2)} == {1, 2}
    assert [f.kernel for f in fwd_launches(rc.CASE_BY_NAME["neg_n204_lds"])] == ["k_dense_fwd_lds<7>", "k_dense_fwd"]
    assert [f.kernel for f in fwd_launches(rc.CASE_BY_NAME["neg_n192"])] == ["k_dense_fwd", "k_dense_fwd"]
    assert fwd_launches(rc.CASE_BY_NAME["s2_k20_ns1_iso"], "grad")[0].copy and not fwd_launches(rc.CASE_BY_NAME["s2_hidden_k36"], "grad")[1].copy


def test_isolation_cases_are_the_ones_the_issue_asks_for():
    names = [c.name for c in ISOLATION]
    assert names == ["s2_k20_ns1_iso", "s2_k64_ns2_rem0_iso", "s1_k20_ns2_iso", "neg_n192", "neg_n204_lds"]
    for c in ISOLATION:
        assert c.P >= 4 and c.P % 2 == 0, c.name          # every even particle has an odd one behind it
    for name in ("s2_k20_ns1_iso", "s1_k20_ns2_iso"):     # (20, 200, 3): 2 400 floats past W, 803 of them the particle's own
        c = rc.CASE_BY_NAME[name]
        assert c.dims == (20, 200, 3) and rc.crosses_particles(c, 1) and rc.crosses_particles(c, 2)
    c = rc.CASE_BY_NAME["s2_k64_ns2_rem0_iso"]
    assert 64 % 32 == 0 and 64 % 16 == 0 and not rc.crosses_particles(c, 1) and not rc.crosses_particles(c, 2)


# ---------------------------------------------------------------- the data
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_data_properties(case):
    x, y, idx, thetas = rc.case_data(case)
    x2, _, _, thetas2 = rc.case_data(case)
    assert np.array_equal(x, x2) and np.array_equal(thetas, thetas2)
    assert thetas.shape == (case.P, case.spec.n_params) and thetas.dtype == np.float32 and x.dtype == np.float32
    assert np.all(np.isfinite(thetas)) and np.all(np.isfinite(x))
    if case.gathered:
        assert idx.shape == (case.batch,) and len(set(idx)) == case.batch and len(x) > case.batch
    else:
        assert idx is None and len(x) == case.batch
    # the last reduction index carries weight: a kernel that drops the tail of K misses by far more than the bound
    l = case.ring_layer
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    for p in (0, case.P - 1):
        w, _ = dc.o_mlp.unpack(thetas[p], case.spec)[l]
        if w.shape[0] > 1:
            assert rms(w[-1]) > 2.0 * rms(w[:-1]), case.name
