"""The SVGD case table (tests/svgd_cases.py) against the library's source and oracle.svgd, on the CPU.

The dispatch of svgd_sweep_impl, svgd_kernel_matrix_impl, svgd_launch_distance_pass and svgd_gram_groups_impl is read out
of pyz_api.hip and pyz_kernels.h and held against `expected_svgd_launches`; the cells the cases reach are compared with
the coverage table name by name; the restated sweep is held bit-equal to oracle.svgd.svgd_step in float64 and float32;
the data of every case is held to what its kind promises (repulsion only, K = I, coupled and balanced); and the
comparisons the GPU matrix uses are run with a float32 stand-in for the device (each must pass, four times inside every
bound) and with every wrong variant (each must fail on every case it applies to)."""

import os
import re

import numpy as np
import pytest

import svgd_cases as sv
from oracle import mlp as o_mlp
from oracle import svgd as o_svgd
from svgd_cases import (CASES, CELLS, DIST_CASES, GROUP_CELLS, MUTATIONS, compare_adam, compare_distances, compare_phi,
                        expected_svgd_launches, reached_cells, ref_sweep, svgd_data)
from test_dense_dispatch_table import CSRC, function_body, src

MARGIN = 4.0   # the float32 stand-in stays this many times inside every bound
IDS = [c.name for c in CASES]


# ---------------------------------------------------------------- the restatement against the source
def test_constants_and_switches_match_the_source():
    ker, api = src("pyz_kernels.h"), src("pyz_api.hip")
    with open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "pyz.h")) as f:
        hdr = f.read()
    assert "#define PYZ_GS_E 3" in ker and sv.GS_RANGE == 256 * 3 and sv.GS_MAX_D == 196608
    assert "#define PYZ_SVGD_PASS 2" in ker and "#define PYZ_SVGD_BLOCK_ELEMS (4 * PYZ_SVGD_PASS * 256)" in ker and sv.ROW_BLOCK == 2048
    assert "#define PYZ_SV_E 128" in ker and sv.SV_E == 128
    from bayesian_inference_for_nn_amd import engine
    assert engine.SVGD_GROUPS == sv.GROUPS
    assert re.search(r"#define PYZ_SVGD_GROUPS\s+8\b", hdr) and "#define PYZ_E_INVALID (-1)" in hdr
    assert "a SEPARATE snapshot" in hdr and "is refused with PYZ_E_INVALID before anything is enqueued" in hdr
    sweep = function_body(api, "static int svgd_sweep_impl(")
    for name, default in sv.ENV_DEFAULTS.items():      # read per call, with these defaults
        text = sweep if name != "PYZ_SVGD_GRAM" else function_body(api, "static int svgd_kernel_matrix_impl(")
        assert f'pyz_env_int("{name}", {default})' in text, name
        assert not re.search(r'static const int \w+ = pyz_env_int\("%s"' % name, api), name
    assert f'pyz_env_int("{sv.ENV_NEVER}", 1 << 20)' in sweep
    assert all(k != sv.ENV_NEVER for c in CASES for k, _ in c.env)
    assert all(set(dict(c.env)) <= set(sv.ENV_DEFAULTS) for c in CASES)
    # the first step of Adam from a zero state leaves phi (1.0f - 0.9f) and phi^2 (1.0f - 0.999f): not float32(0.1), float32(0.001)
    for k in ("__global__ void __launch_bounds__(256) k_svgd_update(", "__global__ void __launch_bounds__(256) k_svgd_update_tile(",
              "void pyz_svgd_gs_adam("):
        body = function_body(ker, k)
        assert "m = m + (phi - m) * (1.0f - 0.9f);" in body and "v = v + (phi * phi - v) * (1.0f - 0.999f);" in body, k
    assert sv.C1 != float(np.float32(0.1)) and sv.C1 == float(np.float32(1.0) - np.float32(0.9))


def test_sweep_dispatch_matches_the_table():
    api = src("pyz_api.hip")
    sweep = function_body(api, "static int svgd_sweep_impl(")
    assert "return n_total <= 64 && row0 % 4 == 0 && n_local % 4 == 0 && d_all != d_particles;" in function_body(api, "static bool svgd_tile_shape(")
    assert "const bool tile_ok = sweep == PYZ_SWEEP_JACOBI && svgd_tile_shape(n_local, n_total, row0, d_all, d_particles);" in sweep
    assert "if (tile_ok && (tiles_on || median)) {" in sweep
    assert sweep.index("svgd_kernel_matrix_impl(m, d_all") < sweep.index("return svgd_combine_impl(m, d_particles")
    assert "const long long gs_range = 256LL * PYZ_GS_E;" in sweep
    assert "if (gs_fused && n_total <= 64 && m->D <= 256 * gs_range) {" in sweep
    assert 'const int gs_reducers = pyz_env_int("PYZ_SVGD_GS_RESIDENT", 1) == 2 ? cdiv(n_total, 8) : cdiv(n_total, 4);' in sweep
    assert "bool resident = gs_res_mode != 0 && ga.nblk + gs_reducers <= pyz_cu_count();" in sweep
    assert "ga.nblk = (int)cdiv(m->D, gs_range);" in sweep
    assert "for (int i = -1; i < n_total; ++i) {" in sweep
    assert "if (zigzag && (i & 1) == 0) PYZ_LAUNCH(k_svgd_gs<true>," in sweep and "else PYZ_LAUNCH(k_svgd_gs<false>," in sweep
    # the per-row arms: one pair of launches for all rows (Jacobi), one pair per row (Gauss-Seidel); k_svgd_loss last
    assert sweep.count("PYZ_LAUNCH(k_svgd_dist,") == 2 and sweep.count("PYZ_LAUNCH(k_svgd_update,") == 2
    assert sweep.index("dim3(nblk, jgroups, n_local)") < sweep.index("for (int i = 0; i < n_local; ++i) {") < sweep.index("dim3(nblk, jgroups, 1)")
    assert sweep.rstrip().endswith("return PYZ_OK;") and sweep.count("PYZ_LAUNCH(k_svgd_loss,") == 2
    res = sweep[sweep.index("if (resident) {\n        pyz_mlp_full"):sweep.index("const int zigzag")]
    assert res.index("PYZ_LAUNCH(k_svgd_gs_resident2,") < res.index("else PYZ_LAUNCH(k_svgd_gs_resident,") < res.index("PYZ_LAUNCH(k_svgd_loss,")
    # the refusal of an in-place Jacobi sweep comes before the gradients are looked at or anything is launched
    assert sweep.index("svgd_check_snapshot(m, d_particles, n_local, d_all, n_total, sweep)") < sweep.index("svgd_check_gradients(") < sweep.index("PYZ_LAUNCH")
    step = function_body(api, "int pyz_svgd_step(")
    assert step.index("svgd_check_snapshot(") < step.index("svgd_gradients_impl(")
    grad = function_body(api, "static int svgd_gradients_impl(")
    assert "if (!fused) PYZ_LAUNCH(k_loss_finalize," in grad
    # the kernel matrix and the distance pass
    km = function_body(api, "static int svgd_kernel_matrix_impl(")
    assert "svgd_launch_distance_pass(L.td, 0, L.td.nblk, gram_on && mfma_f64_layout_ok(st), st);" in km
    assert km.index("svgd_launch_distance_pass(") < km.index("PYZ_LAUNCH(k_svgd_kmat, dim3(n_total), dim3(1024), 0, st, L.td, 1);") \
        < km.index("PYZ_LAUNCH(k_svgd_median,") < km.index("PYZ_LAUNCH(k_svgd_kmat, dim3(n_local), dim3(1024), 0, st, L.ta, 0);")
    lay = function_body(api, "static int svgd_tile_layout(")
    assert "ta.range = PYZ_SV_E * cdiv(m->D, 256LL * PYZ_SV_E);" in lay and "ta.nblk = cdiv(m->D, ta.range);" in lay
    assert "const int dist_rows = median ? n_total : n_local, dist_row0 = median ? 0 : row0;" in lay
    dp = function_body(api, "static void svgd_launch_distance_pass(")
    assert "const int rb_lo = td.row0 >> 4, rb_hi = (td.row0 + td.n_local - 1) >> 4;" in dp
    assert dp.index("if (rb_hi == rb_lo) PYZ_LAUNCH((k_svgd_gram_tile<1, false>)") < dp.index("else if (rb_hi == rb_lo + 1) PYZ_LAUNCH((k_svgd_gram_tile<2, false>)") \
        < dp.index("else PYZ_LAUNCH((k_svgd_gram_tile<4, true>)") < dp.index("PYZ_LAUNCH(k_svgd_dist_tile,")
    assert "PYZ_LAUNCH(k_svgd_update_tile," in function_body(api, "static int svgd_combine_impl(")
    gg = function_body(api, "static int svgd_gram_groups_impl(")
    assert "const int nblk = L.td.nblk, nb8 = cdiv(nblk, PYZ_SVGD_GROUPS);" in gg
    assert "const int blk0 = std::min(g_lo * nb8, nblk), blk1 = std::min(g_hi * nb8, nblk);" in gg
    assert gg.index("if (blk1 > blk0) svgd_launch_distance_pass(L.td, blk0, blk1 - blk0,") < gg.index("PYZ_LAUNCH(k_svgd_group_reduce,")
    assert "svgd_tile_layout(m, d_all, n_total, 0, n_total, 1.0f, L);" in gg


def test_both_distance_kernels_check_the_base_alignment():
    """The 16-byte loads of a row need D % 4 == 0 AND a 16-byte aligned base (the Gram kernel checks its own 8 bytes)."""
    ker = src("pyz_kernels.h")
    for k in ("k_svgd_dist(", "k_svgd_dist_tile("):
        body = function_body(ker, f"__global__ void __launch_bounds__(256) {k}")
        assert "const bool vec_ok = (g.D % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.all) & 15) == 0);" in body, k
        assert body.count("reinterpret_cast<const float4 *>(") - body.count("reinterpret_cast<const float4 *>(&xs") == 1
        assert "vec_ok && d + 3 < g.D" in body
    assert "const bool pair_ok = (g.D % 2 == 0) && ((reinterpret_cast<uintptr_t>(g.all) & 7) == 0);" in ker


def test_expected_launches_of_named_cases():
    by = lambda name, cu=sv.CUS: expected_svgd_launches(sv.CASE_BY_NAME[name], cu)
    assert by("gs_res_w_m7") == ("k_svgd_gs_resident", "k_svgd_loss")
    assert by("gs_res2_w_m12") == ("k_svgd_gs_resident2", "k_svgd_loss")
    assert by("gs_zig_b_m5_rep") == ("k_svgd_gs<false>", "k_svgd_gs<true>", "k_svgd_gs<false>", "k_svgd_gs<true>", "k_svgd_gs<false>",
                                     "k_svgd_gs<true>", "k_svgd_loss")
    assert by("gs_asc_a_m6") == ("k_svgd_gs<false>",) * 7 + ("k_svgd_loss",)
    assert by("gs_rows_a_m65") == ("k_svgd_dist", "k_svgd_update") * 65 + ("k_svgd_loss",)
    assert by("gs_rows_big_m3_rep") == ("k_svgd_dist", "k_svgd_update") * 3 + ("k_svgd_loss",)
    assert by("gs_res_u_m6_unfused")[0] == "k_loss_finalize"
    # the residency gate: 249 blocks + 8 reducers do not fit 256 compute units, 249 + 4 do; a larger part takes both
    big = sv.CASE_BY_NAME["gs_gate_big_m32_rep"]
    assert sv.cdiv(big.D, sv.GS_RANGE) == 249 and big.D == 190810
    assert by("gs_gate_big_m32_rep")[0] == "k_svgd_gs<false>" and len(by("gs_gate_big_m32_rep")) == 34
    assert by("gs_gate_big_m32_rep_res2") == ("k_svgd_gs_resident2", "k_svgd_loss")
    assert by("gs_gate_big_m32_rep", 304) == ("k_svgd_gs_resident", "k_svgd_loss")
    assert sv.CASE_BY_NAME["gs_rows_big_m3_rep"].D == 199555 > sv.GS_MAX_D
    tile = ("k_svgd_kmat", "k_svgd_update_tile")
    assert by("j_gram1_w_shard") == ("k_svgd_gram_tile<1,false>",) + tile
    assert by("j_gram2_b_shard_rep") == ("k_svgd_gram_tile<2,false>",) + tile
    assert by("j_gram4_wm_m64_rep") == by("j_gram4_w_span3") == ("k_svgd_gram_tile<4,true>",) + tile
    assert by("j_gram1_a_m12") == ("k_svgd_gram_tile<1,false>",) + tile      # a whole matrix of 12 rows lies in one row block
    assert by("j_pair_a_m8") == ("k_svgd_dist_tile",) + tile
    assert by("j_med_a_m12") == ("k_svgd_gram_tile<1,false>", "k_svgd_kmat", "k_svgd_median") + tile
    assert by("j_med_b_m64_rep") == ("k_svgd_gram_tile<4,true>", "k_svgd_kmat", "k_svgd_median") + tile
    assert by("j_med_a_m8_pair_shard") == ("k_svgd_dist_tile", "k_svgd_kmat", "k_svgd_median") + tile
    assert by("j_gram_u_shard_unfused") == ("k_loss_finalize", "k_svgd_gram_tile<1,false>") + tile
    for name in ("j_rows_a_m8_switch", "j_rows_a1_m5", "j_rows_a2_row0_2", "j_rows_b_m65_rep", "j_rows_a_m4_off"):
        assert by(name) == ("k_svgd_dist", "k_svgd_update", "k_svgd_loss"), name
    assert sv.svgd_kernels([("(k_svgd_gram_tile<4, true>)", 1.0), ("k_dense_fwd", 2.0), ("k_svgd_gs<true>", 1.0)]) == \
        ("k_svgd_gram_tile<4,true>", "k_svgd_gs<true>")
    assert sv.expected_group_launches(24, 215, 3, 8, True) == ("k_svgd_group_reduce",)
    assert sv.expected_group_launches(24, 215, 0, 3, True) == ("k_svgd_gram_tile<2,false>", "k_svgd_group_reduce")
    assert sv.expected_group_launches(64, 3834, 3, 8, False) == ("k_svgd_dist_tile", "k_svgd_group_reduce")


# ---------------------------------------------------------------- the cases against the table
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_cell_is_reached(cell):
    assert any(cell in reached_cells(c) for c in CASES), f"no case reaches the cell '{cell}'"


@pytest.mark.parametrize("cell", sorted(GROUP_CELLS))
def test_group_cell_is_reached(cell):
    assert any(cell in sv.group_cells(sv.CASE_BY_NAME[n]) for n in DIST_CASES), f"no distance case reaches the cell '{cell}'"


def test_table_and_cases_are_complete():
    assert len(CELLS) == 55 and len(CASES) == 42 and len(MUTATIONS) == 16
    assert set().union(*[reached_cells(c) for c in CASES]) == set(CELLS)
    assert set().union(*[sv.group_cells(sv.CASE_BY_NAME[n]) for n in DIST_CASES]) == set(GROUP_CELLS)
    for c in CASES:
        assert 4 <= c.batch <= 23, c.name
        assert c.median or (float(np.float32(c.gamma)) != 1.0 and c.gamma in (0.37, 2.5)), c.name   # 2 gamma is not 2, exp(-gamma d) not exp(-d)
        assert c.row0 + c.nl <= c.M and (c.sweep == "jacobi" or (c.row0 == 0 and c.nl == c.M)), c.name
        assert not (c.twin and c.median), c.name
        if c.snap_off:
            assert c.sweep == "jacobi" and c.D % 4 == 0, c.name        # the shape whose 16-byte loads the base address decides
        if c.median:
            assert (c.M * c.M) % 2 == 0, c.name                       # always an even count: the mean of the two middle values
        assert c.big == (c.D > 100000), c.name
    for n in DIST_CASES:
        c = sv.CASE_BY_NAME[n]
        assert c.M % 4 == 0 and 4 <= c.M <= 64, n
    # every sweep arm by a repulsion-only case (phi element by element) and by one with a drive
    arms = {}
    for c in CASES:
        arm = (c.sweep, sv.gs_arm(c) if c.sweep == "gs" else sv.jacobi_arm(c) + (" median" if c.median else ""))
        arms.setdefault(arm, set()).add(c.kind)
    assert len(arms) == 7
    for arm, kinds in arms.items():
        assert "rep" in kinds and kinds & {"coupled", "drive"}, (arm, kinds)
    # the gate case reaches two cells from one shape, and on no part both the same
    a, b = sv.CASE_BY_NAME["gs_gate_big_m32_rep"], sv.CASE_BY_NAME["gs_gate_big_m32_rep_res2"]
    assert a._replace(name="", env=()) == b._replace(name="", env=())
    assert "gs per-launch chosen by the residency gate" in reached_cells(a) and "gs resident2 where mode 1 does not fit" in reached_cells(b)


def test_cells_the_older_svgd_tests_reach():
    """What the SVGD tests before this table reach of it, from their shapes (svgd_cases.old_svgd_shapes): the three
    Gauss-Seidel forms, the Gram kernel whole and as shards of one or two row blocks, the pairwise kernel, the per-row
    Jacobi kernels and the median at M = 64 -- always with gamma 1.0 or the median, D even, aligned buffers and a zero Adam
    state, and with no per-element view of phi."""
    old = {name: reached_cells(c) for name, c in sv.old_svgd_shapes().items()}
    # (the kind of data and observable (c) are not properties of a shape: the older tests have neither)
    reached = {c for c in set().union(*old.values()) if not c.startswith(("kind ", "(c) "))}
    missing = CELLS - reached
    assert "jacobi k_svgd_gram_tile<2,false> shard" in old["baseline_shapes::c5[jacobi-gram] shard"]     # rows [32, 64): two row blocks
    for cell in ("gs per-row because M > 64", "gs per-row because D > 196608", "gs per-launch chosen by the residency gate",
                 "gs resident2 where mode 1 does not fit",
                 "jacobi k_svgd_gram_tile<4,true> non-whole range over three row blocks", "jacobi per-row because M > 64",
                 "median M=12 (144 values padded to 256)", "median M=8 (64 values, no padding)",
                 "Gram fetch D odd", "two identical particles", "snapshot 4 bytes off 16-byte alignment: k_svgd_dist",
                 "snapshot 4 bytes off 16-byte alignment: k_svgd_dist_tile", "kind rep", "kind drive", "gamma 0.37", "gamma 2.5",
                 "k_svgd_dist D%4=1", "k_svgd_dist D%4=3", "k_svgd_dist_tile D%4=1", "k_svgd_dist_tile D%4=3",
                 "loss of an unfused head (k_loss_finalize)", "(c) Adam from a non-zero state: gs", "(c) Adam from a non-zero state: jacobi"):
        assert cell in missing, cell
    for cell in ("gs k_svgd_gs_resident", "gs k_svgd_gs_resident2", "gs k_svgd_gs<true/false> alternating", "gs k_svgd_gs<false> only",
                 "gs per-row by switch", "jacobi k_svgd_gram_tile<1,false> shard", "jacobi k_svgd_gram_tile<4,true> whole matrix",
                 "jacobi k_svgd_dist_tile whole matrix (mirrored blocks)", "jacobi k_svgd_dist_tile rectangular shard",
                 "median M=64 (4096 values)", "jacobi per-row by switch", "jacobi per-row because M % 4 != 0", "jacobi per-row because row0 % 4 != 0", "M = 1"):
        assert cell in reached, cell
    print("\n".join(f"OLD | reached | {c}" for c in sorted(reached)) + "\n" + "\n".join(f"OLD | not reached | {c}" for c in sorted(missing)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_data_properties(case):
    a = svgd_data(case)
    M, D, spec = case.M, case.D, case.spec
    assert a.parts.shape == (M, D) and a.parts.dtype == np.float32 and np.all(np.isfinite(a.parts))
    assert a.x.shape == (case.batch, spec.dims[0]) and a.m0.shape == (case.nl, D) == a.v0.shape
    ref = ref_sweep(case, a, a.parts, None, None, 1)
    sq = sv.sq_distances(a.parts)
    off = ~np.eye(M, dtype=bool)
    if case.twin:
        assert np.array_equal(a.parts[0], a.parts[1])
        off[0, 1] = off[1, 0] = False
        assert np.all(ref["k"][0, :2] == 1.0) or case.row0 > 0
    K = np.exp(-ref["gamma"] * sq)
    if case.kind == "drive":
        assert M == 1 or (ref["gamma"] * sq[off]).min() > 800.0
        for il in range(case.nl):      # K is exactly I in float64: phi = g_i / M
            assert np.array_equal(ref["k"][il], np.eye(M)[case.row0 + il]) and np.array_equal(ref["phi"][il], ref["g"][il] / M)
    elif case.kind == "rep":
        ll = sv.last_layer(spec)
        assert np.all(a.parts[:, ll] == 0) and np.all(a.y == 0) and ref["loss"] == 0.0 and np.all(ref["g"] == 0)
        assert np.all(ref["phi"][:, ll] == 0) and np.all(ref["phi"][:, :ll.start] != 0)
    if case.kind != "drive" and not case.big:
        lo, hi = (0.05, 0.9) if case.kind == "coupled" and not (case.median and M > 12) else (1e-3, 0.95)
        assert lo <= K[off].min() and K[off].max() <= hi, (case.name, K[off].min(), K[off].max())
        assert len(np.unique(np.round(K[np.triu(off)], 3))) >= min(6, M * (M - 1) // 2 - 1)     # every K_ij its own weight
    if case.kind == "coupled":
        for il in range(case.nl):      # both terms count in every layer block of every row
            for name, sl in sv.blocks(spec):
                r, d = np.abs(ref["rep"][il, sl]).max(), np.abs(ref["drive"][il, sl]).max()
                assert 0.1 * d <= r <= 10.0 * d, f"{case.name} row {il} block {name}: repulsion {r:.3e} against drive {d:.3e}"
        phi2 = np.abs(ref["phi"]).max() ** 2
        assert np.all(a.m0 != 0) and np.all(a.v0 > 0) and a.v0.max() <= 4.0 * phi2
        for _, sl in sv.blocks(spec):
            s = np.abs(ref["phi"][:, sl]).max()
            assert 0.25 * s * s * 0.999 <= a.v0[:, sl].min() and a.v0[:, sl].max() <= 4.0 * s * s * 1.001
            assert 0.5 * s * 0.999 <= np.abs(a.m0[:, sl]).min() and np.abs(a.m0[:, sl]).max() <= s * 1.001
    assert np.array_equal(svgd_data(case).parts, a.parts) and not a.parts.flags.writeable


# ---------------------------------------------------------------- the restated sweep against oracle.svgd
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", ["gs_res_w_m7", "gs_res_b_m5_rep", "gs_res_a_m3_drive", "j_gram1_a_m12", "j_med_a_m12", "j_rows_a1_m5",
                                  "j_gram_a_m8_twin"])
def test_restated_sweep_equals_the_oracle_module(name, dtype):
    case = sv.CASE_BY_NAME[name]
    assert not case.shard
    data = svgd_data(case)
    sweep = "gauss_seidel" if case.sweep == "gs" else "jacobi"
    for t, m0, v0 in ((1, None, None), (sv.T_ADAM, data.m0, data.v0)):
        if m0 is not None and not sv.has_adam_step(case):
            continue
        st = o_svgd.SVGDState(data.parts, wdtype=dtype)
        if m0 is not None:
            st.m, st.v = m0.astype(dtype), v0.astype(dtype)
        st.t = t - 1
        out = o_svgd.svgd_step(st, data.x, data.y, case.spec, sv.LR, case.gamma if case.median else case.g32, sweep=sweep)
        ref = ref_sweep(case, data, data.parts, m0, v0, t, dtype)
        assert ref["m"].dtype == ref["v"].dtype == dtype
        assert np.array_equal(ref["phi"], out["phi"].astype(np.float64)) and out["phi"].dtype == dtype
        assert np.array_equal(ref["m"], st.m) and np.array_equal(ref["v"], st.v)
        assert np.array_equal(ref["x"], st.particles) and ref["loss"] == out["loss"]


def test_step_size_matches_the_checks_module():
    from svgd_checks import lr_t
    for t in (1, 2, 7):
        assert abs(float(sv.lr_t(t)) - lr_t(sv.LR, t)) <= 1e-15
    assert float(sv.lr_t(7, mutation="lr_t without bias correction")) == sv.LR


# ---------------------------------------------------------------- the comparisons: the stand-in passes, wrong variants fail
def stand_in(case, data, t, mutation=None):
    """A float32 device: the float32 oracle (SVGDState(wdtype=np.float32)'s arithmetic), or for the repulsion-only first
    step -- where the bound is a bound on roundings -- the kernels' own roundings (svgd_cases.kernel_emulation)."""
    if t == 1 and case.kind == "rep" and mutation is None:
        return sv.as_stored(sv.kernel_emulation(case, data, data.parts))
    m0, v0 = (None, None) if t == 1 else (data.m0, data.v0)
    return sv.as_stored(ref_sweep(case, data, data.parts, m0, v0, t, np.float32, mutation=mutation, kernel_consts=True))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_comparison_passes_the_float32_stand_in_and_fails_every_wrong_variant(case):
    data = svgd_data(case)
    rep = {f"(b) {q}": r for q, r in compare_phi(case, data, stand_in(case, data, 1), what="float32 stand-in: ").items()}
    if sv.has_adam_step(case):
        rep.update({f"(c) {q}": r for q, r in compare_adam(case, data, stand_in(case, data, sv.T_ADAM), what="float32 stand-in: ").items()})
    for q, r in sorted(rep.items()):     # (the table of profiles/svgd_matrix/float32_oracle_tolerances.txt: run with -s)
        print(f"FLOAT32 | {case.name} | {case.kind} | {q} | error / tolerance {r:.4f}")
        # (the ulp count and the repulsion-only bound are sums of worst-case roundings: the emulation of those very roundings
        #  stays inside them, not four times inside)
        margin = 1.0 if q == "(b) v ulps" or (q == "(b) phi" and case.kind == "rep") else MARGIN
        if q == "(c) x1":      # (2^-23 |x| is the allowance set for the stored particle, and its own rounding is half of that)
            margin = 2.0
        assert r * margin <= 1.0, f"{case.name}: {q}: the float32 stand-in takes {r:.3f} of the tolerance"
    for mutation in MUTATIONS:
        if not sv.mutation_applies(case, mutation):
            continue
        adam = mutation in sv.ADAM_MUTATIONS
        got = stand_in(case, data, sv.T_ADAM if adam else 1, mutation)
        with pytest.raises(AssertionError):
            (compare_adam if adam else compare_phi)(case, data, got, what=f"wrong variant '{mutation}': ")


def test_every_wrong_variant_is_exercised():
    for mutation in MUTATIONS:
        n = sum(sv.mutation_applies(c, mutation) for c in CASES)
        assert n >= 2, (mutation, n)
    for mutation in ("repulsion without gamma", "exp(-d) instead of exp(-gamma d)"):     # both bandwidths
        assert {c.gamma for c in CASES if sv.mutation_applies(c, mutation)} == {0.37, 2.5}


@pytest.mark.parametrize("name", [n for n in DIST_CASES if not sv.CASE_BY_NAME[n].big])
def test_distance_comparison_passes_float64_forms_and_fails_a_dropped_element(name):
    """Observable (a) with the two forms evaluated in float64 on the host in place of the device."""
    P = sv.dist_parts(sv.CASE_BY_NAME[name]).astype(np.float64)
    pair = sv.sq_distances(P[:, ::-1])                 # (another summation order)
    G = P @ P.T
    n2 = np.einsum("id,id->i", P, P)
    gram = (n2[:, None] + n2[None, :]) - 2.0 * G
    gram = 0.5 * (gram + gram.T)
    for form, got in (("pairwise", pair), ("gram", gram)):
        for q, r in compare_distances(P, got, form, what=name).items():
            print(f"FLOAT64 | {name} | {q} | error / tolerance {r:.4f}")
            assert r * MARGIN <= 1.0
        with pytest.raises(AssertionError):
            compare_distances(P, sv.sq_distances(P[:, :-1]) if form == "pairwise" else gram - (P[:, -1:] - P[None, :, -1]) ** 2, form,
                              what=sv.DIST_MUTATION)
    asym = pair.copy()
    asym[0, 1] = np.nextafter(asym[0, 1], 1.0)
    with pytest.raises(AssertionError):
        compare_distances(P, asym, "pairwise")
