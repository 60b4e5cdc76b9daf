"""The Dense case table (tests/dense_cases.py) against the library's source, on the CPU.

The constants and expressions of the launch decisions are read out of pyz_gemm.h, pyz_gemm_ring.h and pyz_api.hip and
compared with the plain-Python restatement; the wave-count boundaries are pinned as literal values; the cells the cases
reach are compared with the coverage table cell by cell, so deleting a case or moving a threshold fails here with the
name of the lost cell; and the data of every case is checked to be what the GPU matrix relies on."""

import os
import re

import numpy as np
import pytest

import dense_cases as dc
from dense_cases import CASES, CELLS, case_data, expected_launches, pick_waves, reached_cells, reference_stats

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesian_inference_for_nn_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def squash(s):
    return re.sub(r"\s+", "", s)


def env_default(text, name):
    m = re.findall(r'pyz_env_int\("%s",\s*(-?\d+)\)' % re.escape(name), text)
    assert m, f"no pyz_env_int(\"{name}\", ...) found"
    assert len(set(m)) == 1, (name, m)
    return int(m[0])


def function_body(text, head):
    """The text from `head` to the closing brace of that function (top-level functions end with a brace in column 0)."""
    i = text.index(head)
    return text[i:text.index("\n}", i)]


# ---------------------------------------------------------------- the restatement against the source
def test_environment_defaults_match_the_source():
    gemm, ring, api = src("pyz_gemm.h"), src("pyz_gemm_ring.h"), src("pyz_api.hip")
    assert env_default(gemm, "PYZ_WAVES_TARGET") == dc.WAVES_TARGET
    assert env_default(gemm, "PYZ_MIN_STEPS") == dc.MIN_STEPS
    assert env_default(gemm, "PYZ_FWD_LDS_MAXROWS") == dc.LDS_MAXROWS
    assert env_default(gemm, "PYZ_FWD_LDS_MINWG") == dc.LDS_MINWG
    assert env_default(gemm, "PYZ_FWD_LDS") == 1
    assert env_default(ring, "PYZ_FWD_RING") == 1
    assert env_default(ring, "PYZ_FWD_RING_MINWG") == dc.RING_MINWG
    assert env_default(ring, "PYZ_FWD_RING_MAXWG") == dc.RING_MAXWG
    assert env_default(ring, "PYZ_FWD_RING_WIDE") == 0
    assert env_default(api, "PYZ_GATHER_COPY") == 1
    # read once per process (static): the GPU module refuses to run with them set
    for name, text in (("PYZ_WAVES_TARGET", gemm), ("PYZ_MIN_STEPS", gemm), ("PYZ_GATHER_COPY", api)):
        assert re.search(r'static const int \w+ = pyz_env_int\("%s"' % name, text), name
        assert name in dc.ENV_FORBIDDEN
    # read per call: cases may set them
    for name in ("PYZ_FWD_LDS", "PYZ_FWD_LDS_MINWG"):
        assert not re.search(r'static const int \w+ = pyz_env_int\("%s"' % name, gemm), name


def test_pick_waves_and_step_counts_match_the_source():
    gemm, api = src("pyz_gemm.h"), src("pyz_api.hip")
    body = squash(function_body(gemm, "static inline int pyz_pick_waves("))
    assert "intS=1;while(S<16&&tiles*S<target&&mfma_steps/(2*S)>=min_steps)S*=2;returnS;" in body
    assert "static inline unsigned pyz_pad8(long long n, int P) { return (unsigned)(P > 1 ? (n + 7) / 8 * 8 : n); }" in gemm
    fwd = squash(function_body(gemm, "static inline void pyz_launch_fwd("))
    assert "tiles=(longlong)((grid_batch+31)/32)*((g.N+31)/32);" in fwd
    assert "pyz_pick_waves(tiles*P,(g.K+1)/2+1)" in fwd
    assert "PYZ_LAUNCH(k_dense_fwd,dim3(pyz_pad8(tiles,P),P),dim3(64*S)" in fwd
    for nt in (2, 4, 7):
        assert f"PYZ_LAUNCH(k_dense_fwd_lds<{nt}>,grid,block,0,st,g)" in fwd
    bd = squash(function_body(gemm, "static inline void pyz_launch_bwd_data("))
    assert "tiles=(longlong)((grid_batch+31)/32)*((g.K+31)/32);" in bd and "pyz_pick_waves(tiles*P,(g.N+1)/2)" in bd
    bw = squash(function_body(gemm, "static inline void pyz_launch_bwd_weight("))
    assert "tiles=(longlong)((g.K+1+31)/32)*((g.N+31)/32);" in bw and "pyz_pick_waves(tiles*P,(grid_batch+1)/2)" in bw
    wa = squash(function_body(api, "void launch_wgrad_all("))
    assert "pyz_pick_waves((longlong)tiles*P,(grid_batch+1)/2)" in wa
    assert "tiles+=((ly.K+1+31)/32)*((ly.N+31)/32);" in squash(function_body(api, "int wgrad_layers("))


def test_wgrad_all_switch_arms_match_the_source():
    body = function_body(src("pyz_api.hip"), "void launch_wgrad_all(")
    arms = [int(s) for s in re.findall(r"case (\d+):", body)]
    assert "default:" in body
    launched = re.findall(r"PYZ_LAUNCH\(\(?(k_wgrad_all<[^>]*>)\)?,", body)
    assert sorted(arms + [16]) == list(dc.WGRAD_ALL_S), arms
    assert launched == ["k_wgrad_all<1, true>", "k_wgrad_all<1>", "k_wgrad_all<2>", "k_wgrad_all<4>", "k_wgrad_all<8>",
                        "k_wgrad_all<16>"], launched
    assert "if (a.mode == PYZ_UPD_NONE) PYZ_LAUNCH((k_wgrad_all<1, true>)" in body
    assert [dc.wgrad_all_expr(S, True) for S in dc.WGRAD_ALL_S] == ["k_wgrad_all<1, true>", "k_wgrad_all<2>",
                                                                    "k_wgrad_all<4>", "k_wgrad_all<8>", "k_wgrad_all<16>"]
    assert dc.wgrad_all_expr(1, False) == "k_wgrad_all<1>"


def test_vec_fuse_lds_and_ring_conditions_match_the_source():
    gemm, ring, api = src("pyz_gemm.h"), src("pyz_gemm_ring.h"), src("pyz_api.hip")
    assert "g.vec = (g.K % 8 == 0) && aligned16(g.in) ? 1 : 0;" in function_body(api, "DenseArgs forward_args(")
    vec_bwd = "g.vec = (N % 8 == 0) && (m->w_off[l] % 4 == 0) && (P == 1 || theta_ps % 4 == 0) && aligned16(theta) ? 1 : 0;"
    assert vec_bwd in function_body(api, "void launch_backward(")
    assert vec_bwd in function_body(api, "void launch_bwd_data_hidden(")
    assert "inline bool can_fuse(const pyz_mlp *m) { return m->dims[m->L] <= %d; }" % dc.FUSE_MAX_N in api
    assert "float *xb = (use_xb && want_grad && row_idx && m->L > 1) ? m->xb : nullptr;" in api
    assert "if (!g.row_idx && !g.init_on && !g.gather_out) g.rows_cap = std::min(grid_batch, m->max_batch);" in api
    lds = squash(function_body(gemm, "static inline bool pyz_fwd_takes_lds("))
    assert "lds_ok=g.K%4==0&&g.N%2==0&&g.lda%4==0&&g.w_off%2==0&&(P==1||g.theta_pstride%2==0)&&(P==1||g.in_pstride%4==0)" in lds
    nt = "constintNT=g.N<=%d?2:(g.N<=%d?4:7);" % dc.LDS_NT_N
    assert nt in lds and nt in squash(function_body(gemm, "static inline void pyz_launch_fwd("))
    assert "wg128=(longlong)((grid_batch+127)/128)*((g.N+32*NT-1)/(32*NT))*P;" in lds
    assert ("returnS==1&&!g.gate&&lds_on&&lds_ok&&g.N>=%d&&grid_batch>=%d&&(grid_batch<=lds_max_rows||P>=%d)&&"
            "wg128>=pyz_env_int(\"PYZ_FWD_LDS_MINWG\",%d);" % (dc.LDS_MIN_N, dc.LDS_MIN_ROWS, dc.LDS_MANY_P, dc.LDS_MINWG)) in lds
    assert "const bool wide = (N & 3) == 0 && (g.out_pstride & 3) == 0 && (reinterpret_cast<uintptr_t>(g.out) & 15) == 0;" in gemm
    rv = function_body(ring, "static inline int pyz_fwd_ring_variant(")
    assert "if (wgs < min_wg || wgs > max_wg) return 0;" in rv
    assert "if (g.K % 4 || g.N % 4 || g.lda % 4 || g.w_off % 4 || (P > 1 && g.in_pstride % 4)) return 0;" in rv
    assert "if (g.N > %d && g.N <= %d) return 1;" % dc.RING_N in rv
    assert "const int n_cg = g.N > 200 ? (g.N + 199) / 200 : 1;" in rv


# ---------------------------------------------------------------- literal boundaries
def first_k_with(S, fn):
    return next(k for k in range(1, 2000) if fn(k)[0] == S)


def test_wave_count_boundaries_are_pinned():
    """Batch 70, N = 40 (6 forward tiles): the first K / N / batch that gives each S."""
    fwd = lambda K: pick_waves(dc.fwd_tiles(70, 40), dc.fwd_steps(K))
    bwd = lambda N: pick_waves(dc.bwd_data_tiles(70, 40), dc.bwd_data_steps(N))
    wg = lambda B: pick_waves(dc.wgrad_tiles(40, 40), dc.wgrad_steps(B))
    assert [first_k_with(S, fwd) for S in (1, 2, 4, 8, 16)] == [1, 29, 61, 125, 253]
    assert [fwd(K)[0] for K in (28, 29, 60, 61, 124, 125, 252, 253, 4000)] == [1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [first_k_with(S, bwd) for S in (1, 2, 4, 8, 16)] == [1, 31, 63, 127, 255]
    assert [bwd(N)[0] for N in (16, 30, 31, 62, 63, 126, 127, 254, 255)] == [1, 1, 2, 2, 4, 4, 8, 8, 16]
    assert [first_k_with(S, wg) for S in (1, 2, 4, 8, 16)] == [1, 31, 63, 127, 255]
    assert [wg(B)[0] for B in (16, 30, 31, 62, 63, 126, 127, 254, 255)] == [1, 1, 2, 2, 4, 4, 8, 8, 16]
    assert all(fwd(K)[1] == "steps" for K in (28, 29, 61, 125)) and fwd(253)[1] == "cap"


def test_tile_limited_exits_are_pinned():
    assert pick_waves(dc.fwd_tiles(4096, 200), dc.fwd_steps(784)) == (4, "tiles")
    assert pick_waves(dc.fwd_tiles(1024, 208) * 8, dc.fwd_steps(784)) == (2, "tiles")
    assert dc.fwd_ring_variant(784, 200, 1024, 8, 0, True) == 1      # 193 .. 200 columns: that launch takes the ring
    assert dc.fwd_ring_variant(784, 208, 1024, 8, 0, True) == 0
    mnist = sum(dc.wgrad_tiles(K, N) for K, N in ((784, 400), (400, 400), (400, 10)))
    assert pick_waves(mnist, dc.wgrad_steps(1024)) == (8, "tiles")
    assert pick_waves(3072, 10 ** 6) == (1, "tiles") and pick_waves(3071, 10 ** 6)[0] == 2
    assert pick_waves(1, 15) == (1, "steps") and pick_waves(1, 16) == (2, "steps")
    assert [dc.pad8(n, P) for n, P in ((9, 1), (9, 2), (16, 2), (17, 64))] == [9, 16, 16, 24]
    assert [dc.lds_nt(N) for N in (48, 64, 65, 128, 129, 224, 500)] == [2, 2, 4, 4, 7, 7, 7]


def test_lds_rule_at_its_edges():
    take = lambda **kw: dc.fwd_takes_lds(**{**dict(K=16, N=64, batch=512, P=64, D=4522, w_off=0, S=1, in_aligned16=True), **kw})
    assert take()
    assert not take(S=2) and not take(N=46) and not take(batch=127, min_wg=1) and not take(K=18) and not take(N=63)
    assert not take(P=63) and take(P=63, min_wg=252) and not take(lds_on=0) and not take(in_aligned16=False)
    assert not take(D=4521) and take(D=4521, P=1, min_wg=1) and not take(w_off=3)
    assert not take(batch=2049, P=7, min_wg=1) and take(batch=2049, P=8, min_wg=1)


# ---------------------------------------------------------------- the cases against the table
def test_cases_reach_every_cell_of_the_table():
    by_cell = {}
    for c in CASES:
        for cell in reached_cells(c):
            by_cell.setdefault(cell, []).append(c.name)
    lost = sorted(CELLS - set(by_cell))
    assert not lost, f"cells no case reaches: {lost}"
    assert set(by_cell) == set(CELLS)


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_cell_is_reached(cell):
    assert any(cell in reached_cells(c) for c in CASES), f"no case reaches the cell '{cell}'"


def test_no_case_went_missing():
    """Several cells are reached by more than one case (other edges differ): removing one of those loses no cell, so the
    count is pinned as well."""
    assert len(CASES) == 64 and len({c.name for c in CASES}) == 64


def test_table_has_the_cells_the_issue_lists():
    assert len(CELLS) == 109
    for fam, n in (("fwd ", 37), ("copy ", 6), ("rows_cap ", 2), ("lds ", 13), ("bwd_data ", 20), ("bwd_weight ", 15),
                   ("wgrad_all ", 16)):
        assert sum(c.startswith(fam) for c in CELLS) == n, fam


def test_no_case_takes_the_ring_and_every_case_is_small():
    for c in CASES:
        for call in ("grad", "forward"):
            for B in (c.batch, max(c.batch - 1, 1)):
                expected_launches(c, B, call)          # asserts pyz_fwd_ring_variant == 0 for every forward layer
        assert c.max_batch * max(c.dims) * 4 < 2 ** 31, c.name     # batch x row bytes: the buffer descriptors' range
        assert c.P <= 64 and c.batch <= 1024 and c.P * c.max_batch * max(c.dims) <= 64 * 1024 * 1024 // 4, c.name
        assert set(c.env) <= {"PYZ_FWD_LDS", "PYZ_FWD_LDS_MINWG"}, c.name
        assert not (c.sgd and (c.P > 1 or not dc.can_fuse(c.dims))), c.name


def test_expected_launches_of_known_shapes():
    la = expected_launches(dc.CASE_BY_NAME["lds_default_p64"])
    assert [f.kernel for f in la.fwd] == ["k_dense_fwd_lds<4>", "k_dense_fwd_lds<4>"] and la.fwd[0].copy and not la.fwd[1].copy
    assert [w.kernel for w in la.wgrad] == ["k_wgrad_all<4>"] and la.wgrad[0].gather == "copy" and len(la.bwd_data) == 1
    la = expected_launches(dc.CASE_BY_NAME["unf_n255_three_hidden"])
    assert [f.kernel for f in la.fwd] == ["k_dense_fwd"] * 4 and [b.S for b in la.bwd_data] == [16, 2, 2]
    assert [w.kernel for w in la.wgrad] == ["k_dense_bwd_weight"] * 4
    la = expected_launches(dc.CASE_BY_NAME["wg_l1_self_gather"])
    assert la.fwd == [] and la.bwd_data == [] and la.wgrad[0].gather == "self"
    assert expected_launches(dc.CASE_BY_NAME["wg_sgd_s1"]).wgrad[0].kernel == "k_wgrad_all<1>"
    assert expected_launches(dc.CASE_BY_NAME["fwd_k24_s1_vec_n31_b1"]).wgrad[0].kernel == "k_wgrad_all<1, true>"
    assert len(expected_launches(dc.CASE_BY_NAME["fwd_k64_s4_vec_n70"], call="forward").fwd) == 2   # forward(): every layer


# ---------------------------------------------------------------- the data
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_data_properties(case):
    x, y, idx, thetas = case_data(case)
    x2, y2, idx2, thetas2 = case_data(case)
    assert np.array_equal(x, x2) and np.array_equal(y, y2) and np.array_equal(thetas, thetas2)
    spec, B = case.spec, case.batch
    assert thetas.shape == (case.P, spec.n_params) and thetas.dtype == np.float32 and x.dtype == np.float32
    assert np.all(np.isfinite(thetas)) and np.all(np.isfinite(x))
    if case.gathered:
        assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < len(x) and len(x) > B and len(set(idx)) == B
    else:
        assert idx is None and len(x) == B
    rows = x if idx is None else x[idx]
    # edge weighting: the last input column, the last batch row and the last row of every W are about 8 times the rest
    # (the rms of one row of a dozen normal draws is itself uncertain by a quarter: within a factor of three of 8)
    lo, hi = dc.EDGE / 3.0, dc.EDGE * 3.0
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    if spec.dims[0] > 1 and B > 1:
        assert lo < rms(rows[:-1, -1]) / rms(rows[:-1, :-1]) < hi
        assert lo < rms(rows[-1, :-1]) / rms(rows[:-1, :-1]) < hi
    for p in range(case.P):
        for (w, b), K in zip(dc.o_mlp.unpack(thetas[p], spec), spec.dims[:-1]):
            if K > 1:
                assert lo < rms(w[-1]) / rms(w[:-1]) < hi, case.name
    within, dead = reference_stats(case)
    for l, act in enumerate(spec.acts):
        if act in ("tanh", "sigmoid"):
            assert within[l] >= 0.9, f"{case.name}: layer {l} ({act}): only {within[l]:.2f} of the pre-activations within +-4"
        if act == "relu":
            assert dead[l] <= 0.5, f"{case.name}: layer {l}: {dead[l]:.2f} of the relu units dead over the batch"
