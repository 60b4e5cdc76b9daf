"""The ADAM / VADAM / BSAM case table (tests/adam_bsam_cases.py) against the library's source and the restatements of
tests/adam_checks.py and tests/bsam_checks.py, on the CPU.

Which kernels each step launches on the fused and the unfused path, their wave counts, LDS bytes and grids, the group order
of k_dense_bwd_weight_sq, when layer 0 reads the batch copy and the Philox streams are read out of pyz_api.hip, pyz_gemm.h,
pyz_kernels.h and pyz_rng.h; the cells the cases reach are compared with the coverage table name by name; the restated steps
are held bit-equal to AdamRef / BsamRef in float64; and the comparison the GPU matrix uses is run with the float32
restatement in place of the device (it must pass, four times inside every bound) and with every wrong restatement (each
must fail on every case and kind it applies to)."""

import re

import numpy as np
import pytest

import adam_bsam_cases as ab
import adam_checks as ac
import bsam_checks as bc
import dense_cases as dc
from adam_bsam_cases import CASES, CELLS, KINDS, MUTATIONS, ab_data, compare_step, expected_ab_launches, reached_cells, ref_step
from test_dense_dispatch_table import function_body, squash, src

CPU_VARIANTS = {"adam": ("plain",), "vadam": ("injected", "device"), "bsam": ("injected", "device")}
MARGIN = 4.0   # the float32 restatement stays this many times inside every bound (test_step_dispatch_table.MARGIN)


# ---------------------------------------------------------------- the restatement against the source
def test_streams_match_the_source():
    rng = src("pyz_rng.h")
    from bayesian_inference_for_nn_amd import _lib
    for kind, const in (("vadam", "PYZ_STREAM_VADAM"), ("bsam", "PYZ_STREAM_BSAM")):
        m = re.search(r"#define\s+%s\s+(\d+)u?" % const, rng) or re.search(r"%s\s*=\s*(\d+)" % const, rng)
        assert m, const
        assert int(m.group(1)) == ab.STREAM[kind] == getattr(_lib, const[4:])
    ker = src("pyz_kernels.h")
    assert "pyz_normal4(seed, PYZ_STREAM_VADAM, step, (uint64_t)t)" in function_body(ker, "void pyz_vadam_perturb_elems(")
    assert "pyz_normal4(seed, PYZ_STREAM_BSAM, step, (uint64_t)t)" in function_body(ker, "void pyz_bsam_perturb_elems(")


def test_wgrad_launchers_pick_the_arms_the_table_says():
    api = src("pyz_api.hip")
    adam = function_body(api, "void launch_wgrad_adam(")
    assert "const int tiles = wgrad_layers(m, 1, x, row_idx, ctl, a.w, gathered);" in adam
    assert "const int S = pyz_pick_waves(tiles, (grid_batch + 1) / 2);" in adam and "const dim3 grid(tiles + 1);" in adam
    for S in ab.SS:
        arm = "default:" if S == 16 else f"case {S}:"
        lds = "0" if S == 1 else f"{S} * 4096"
        assert f"{arm} PYZ_LAUNCH({ab.wgrad_adam_expr(S)}, grid, dim3({64 * S}), {lds}, st, a); break;" in adam, S
        assert ab.wgrad_lds_bytes(S) == (0 if S == 1 else eval(lds))
    assert adam.count("PYZ_LAUNCH(") == 5
    bsam = function_body(api, "void launch_wgrad_bsam(")
    assert "const int tiles = wgrad_layers(m, 1, x, row_idx, ctl, a.w, gathered);" in bsam
    assert "const int S = pyz_pick_waves(tiles, (grid_batch + 1) / 2);" in bsam and "const dim3 grid(tiles + 1);" in bsam
    assert "if (phase == 0) PYZ_LAUNCH((k_wgrad_bsam<W, 0>), grid, dim3(64 * W), LDS, st, a);" in bsam
    assert "else PYZ_LAUNCH((k_wgrad_bsam<W, 1>), grid, dim3(64 * W), LDS, st, a);" in bsam
    for S in ab.SS:
        arm = "default:" if S == 16 else f"case {S}:"
        lds = "0" if S == 1 else f"{S} * 4096"
        assert f"{arm} PYZ_BSAM_CASE({S}, {lds});" in bsam, S
    assert ab.wgrad_bsam_expr(4, 1) == "k_wgrad_bsam<4, 1>"
    # the tile count both hand to pyz_pick_waves is the sum over layers dense_cases.wgrad_tiles restates
    assert "tiles += ((ly.K + 1 + 31) / 32) * ((ly.N + 31) / 32);" in function_body(api, "int wgrad_layers(")
    # the probe drops the parentheses a launch site wraps a template kernel in
    assert "const bool wrapped = nm[0] == '(';" in function_body(api, "int pyz_probe_end(")


def test_step_functions_launch_what_the_table_says():
    api, ker, gemm = src("pyz_api.hip"), src("pyz_kernels.h"), src("pyz_gemm.h")
    lb = function_body(api, "void launch_loss_backward(")
    # can_fuse decides between launch_wgrad_adam and launch_backward(..., m->grad2)
    assert lb.index("if (can_fuse(m)) {") < lb.index("if (adam) launch_wgrad_adam(m, x, row_idx, grid_batch, ctl, *adam, st, xb);") \
        < lb.index("flush_ctl(m, st);") < lb.index("launch_backward(m, theta, theta_ps, P, x, row_idx, grid_batch, ctl, upd.grad, st, adam ? m->grad2 : nullptr);")
    assert "inline bool can_fuse(const pyz_mlp *m) { return m->dims[m->L] <= 32; }" in api and dc.FUSE_MAX_N == 32
    # xb (gather "copy") only with row_idx and L > 1
    assert "float *xb = (use_xb && want_grad && row_idx && m->L > 1) ? m->xb : nullptr;" in lb
    bp = function_body(api, "void launch_bsam_pass(")
    assert "float *xb = (use_xb && row_idx && m->L > 1) ? m->xb : nullptr;" in bp
    assert bp.index("launch_forward(") < bp.index("launch_head(") < bp.index("launch_bwd_data_hidden(") \
        < bp.index("launch_wgrad_bsam(m, x, row_idx, grid_batch, m->ctl, phase, a, st, xb);")
    wl = function_body(api, "int wgrad_layers(")
    assert "ly.in = (row_idx && gathered) ? gathered : x;" in wl and "ly.gather = (row_idx && !gathered) ? 1 : 0;" in wl
    # the unfused weight gradients: the squared kernel when grad_sq is given, layers from the last to the first
    bw = function_body(api, "void launch_backward(")
    assert "for (int l = m->L - 1; l >= 0; --l) {" in bw
    assert "if (grad_sq) pyz_launch_bwd_weight_sq(g, grad_sq, grid_batch, st);\n    else pyz_launch_bwd_weight(g, grid_batch, P, st);" in bw
    sq = squash(function_body(gemm, "static inline void pyz_launch_bwd_weight_sq("))
    assert "tiles=(longlong)((g.K+1+31)/32)*((g.N+31)/32);" in sq and "pyz_pick_waves(tiles,(grid_batch+1)/2)" in sq
    assert "PYZ_LAUNCH(k_dense_bwd_weight_sq,dim3((unsigned)tiles),dim3(64*S),S>1?S*4096:0,st,g,out2)" in sq
    # pyz_adam_step
    adam = function_body(api, "int pyz_adam_step(")
    assert "const bool fused = can_fuse(m);" in adam
    assert "launch_loss_backward(m, d_theta, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, a.w, st, -1, &a);" in adam
    assert "if (!fused)\n    PYZ_LAUNCH(k_adam_update, dim3(cdiv(m->D, 256)), dim3(256), 0, st, d_theta, d_m, d_v, m->grad, m->grad2, m->D, a.a," in adam
    assert adam.count("PYZ_LAUNCH(") == 1
    pert = function_body(api, "int pyz_vadam_perturb(")
    assert "PYZ_LAUNCH(k_vadam_perturb, dim3(cdiv(cdiv(m->D, 4), 256)), dim3(256), 0, as_stream(stream), d_theta, d_v, m->D, lam," in pert
    assert pert.count("PYZ_LAUNCH(") == 1
    # pyz_bsam_step: the perturbation, then two passes
    bsam = function_body(api, "int pyz_bsam_step(")
    assert "PYZ_LAUNCH(k_bsam_perturb, dim3(cdiv(cdiv(m->D, 4), 256)), dim3(256), 0, st, d_theta, d_v, m->D, a.a.inv_n, seed," in bsam
    order = [bsam.index(t) for t in (
        "PYZ_LAUNCH(k_bsam_perturb", "if (fused) {",
        "launch_bsam_pass(m, d_theta, d_x, d_y, d_row_idx, batch, 0, a, st);",
        "launch_bsam_pass(m, d_theta, d_x, d_y, d_row_idx, batch, 1, a, st);", "} else {",
        "const dim3 grid(cdiv(m->D, 256)), block(256);", "PYZ_LAUNCH(k_bsam_ascent, grid, block, 0, st,",
        "PYZ_LAUNCH(k_bsam_update, grid, block, 0, st,")]
    assert order == sorted(order)
    unfused = bsam[bsam.index("} else {"):]
    call = "launch_loss_backward(m, d_theta, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, a.w, st);"
    assert unfused.count(call) == 2 and unfused.index(call) < unfused.index("PYZ_LAUNCH(k_bsam_ascent") < unfused.rindex(call) \
        < unfused.index("PYZ_LAUNCH(k_bsam_update")
    # one or four elements per thread
    for k, per in ab.PER_THREAD.items():
        body = function_body(ker, f"__global__ void {k}(")
        if per == 1:
            assert "const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;" in body, k
    for fn in ("void pyz_vadam_perturb_elems(", "void pyz_bsam_perturb_elems("):
        body = function_body(ker, fn)
        assert "const long long e0 = 4 * t;" in body and "if (e0 >= D) return;" in body
    assert "pyz_vadam_perturb_elems(theta, v, D, lam, num_data, seed, step, eps);" in function_body(ker, "__global__ void k_vadam_perturb(")
    assert "pyz_bsam_perturb_elems(theta, v, D, inv_n, seed, step, eps);" in function_body(ker, "__global__ void k_bsam_perturb(")
    assert [ab.update_grid("k_adam_update", D) for D in (1, 256, 257, 2596)] == [1, 1, 2, 11]
    assert [ab.update_grid("k_bsam_perturb", D) for D in (1, 1024, 1025, 2596)] == [1, 1, 2, 3]


def test_squared_weight_gradient_walks_16_4_1():
    gemm = src("pyz_gemm.h")
    body = function_body(gemm, "__global__ void k_dense_bwd_weight_sq(")
    for gather in ("true", "false"):
        at = [body.index(f"pyz_wgrad_steps<{G}, {gather}, true>(s, se, acc,") for G in ab.GROUPS]
        assert at == sorted(at), gather
    assert body.index("if (idx) {") < body.index("pyz_wgrad_steps<16, true, true>") < body.index("} else {") \
        < body.index("pyz_wgrad_steps<16, false, true>")
    assert "const int32_t *idx = g.row_idx ? g.row_idx + g.ctl->row_off : nullptr;" in body
    assert "int s = (steps * w) / S;" in body and "const int se = (steps * (w + 1)) / S;" in body and "const int steps = (batch + 1) >> 1;" in body
    assert "for (; s + G <= se; s += G) {" in function_body(gemm, "void pyz_wgrad_steps(")
    assert ab.groups_of(21) == {16, 4, 1} and ab.groups_of(20) == {16, 4} and ab.groups_of(10) == {4, 1} and ab.groups_of(3) == {1}
    assert ab.wave_ranges(336, 16)[:2] == [(0, 21), (21, 42)] and {e - s for s, e in ab.wave_ranges(336, 16)} == {21}


def test_fused_kernels_keep_the_paths_the_cells_name():
    """k_wgrad_adam: gathered rows in a loop of its own, else pyz_wgrad_accumulate_sq, whose odd last row is peeled."""
    fused = src("pyz_fused.h")
    adam = function_body(fused, "k_wgrad_adam(std::conditional_t<CHAIN, AdamRunArgs, AdamArgs> A) {")
    assert "const int32_t *idx = (ly.gather && g.row_idx) ? g.row_idx + g.ctl->row_off : nullptr;" in adam
    assert adam.index("if (idx) {") < adam.index("acc2 = pyz_mfma(a * a, gd * gd, acc2);") < adam.index("pyz_wgrad_accumulate_sq(acc, acc2, fb,")
    assert "pyz_adam_math(A.a, th0[q], m0[q], v0[q], gv[q], sv[q] / fb)" in adam and "const float fb = (float)batch;" in adam
    acc = function_body(fused, "void pyz_wgrad_accumulate_sq(")
    assert "const int full = batch >> 1;" in acc and "if (se > full) {" in acc
    bsam = function_body(fused, "k_wgrad_bsam(std::conditional_t<CHAIN, BsamRunArgs, BsamArgs> A) {")
    assert bsam.index("if (idx) {") < bsam.index("pyz_wgrad_accumulate(acc, ly.in, ic, ly.delta, n, ly.lda, N, batch, s, se, h, is_w, is_b, prefetch);")


def test_launches_follow_the_dense_table():
    for c in CASES:
        for kind in KINDS:
            la = expected_ab_launches(c, kind)
            assert la.perturb == ((ab.PERTURB_KERNEL[kind],) if kind != "adam" else ())
            if c.fused:
                tiles = sum(dc.wgrad_tiles(K, N) for K, N in zip(c.dims[:-1], c.dims[1:]))
                S, _ = dc.pick_waves(tiles, dc.wgrad_steps(c.batch))
                assert la.S == S and S in ab.SS and la.sq == ()
                assert la.sequence == ((f"k_wgrad_bsam<{S}, 0>", f"k_wgrad_bsam<{S}, 1>") if kind == "bsam" else (f"k_wgrad_adam<{S}>",))
            else:
                assert la.S == 0 and c.dims[-1] > dc.FUSE_MAX_N
                if kind == "bsam":
                    assert la.sequence.count("k_dense_bwd_weight") == 2 * c.L and la.sequence[c.L] == "k_bsam_ascent" \
                        and la.sequence[-1] == "k_bsam_update" and len(la.sequence) == 2 * c.L + 2
                else:
                    assert la.sequence == ("k_dense_bwd_weight_sq",) * c.L + ("k_adam_update",)
                    assert [q.layer for q in la.sq] == list(range(c.L - 1, -1, -1))
    by = lambda name, kind="adam": expected_ab_launches(ab.CASE_BY_NAME[name], kind)
    assert by("f_s1").sequence == ("k_wgrad_adam<1>",) and by("f_s16_l3_mse", "bsam").sequence == ("k_wgrad_bsam<16, 0>", "k_wgrad_bsam<16, 1>")
    assert by("f_b1").S == by("f_b2").S == 1 and by("f_tiles_2x3").S == 2
    assert by("f_s4_copy").gather == "copy" and by("f_s4_self_l1").gather == "self" and by("u_d218_self").gather == "self"
    # the wave of 21 steps: S = 16 by the cap, 336 steps
    for name, gather in (("u_g16_plain", "none"), ("u_g16_self", "self")):
        (q,) = by(name).sq
        assert (q.S, set(q.waves), q.groups, q.gather) == (16, {21}, frozenset({16, 4, 1}), gather)
        assert dc.pick_waves(dc.wgrad_tiles(q.K, q.N), dc.wgrad_steps(671)) == (16, "cap")
    # ... which the six models of the older tests never reach: batches of 40 and 33 at S = 2, ragged ends at S = 1
    for batch in (40, 33, 11, 4):
        for K, N in ((12, 20), (20, 40), (9, 16), (16, 48)):
            S, _ = dc.pick_waves(dc.wgrad_tiles(K, N), dc.wgrad_steps(batch))
            assert 16 not in set().union(*[ab.groups_of(e - s) for s, e in ab.wave_ranges(dc.wgrad_steps(batch), S)])


# ---------------------------------------------------------------- the cases against the table
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_cell_is_reached(cell):
    assert any(cell in reached_cells(c) for c in CASES), f"no case reaches the cell '{cell}'"


def test_table_and_cases_are_complete():
    assert len(CELLS) == 55 and len(CASES) == 18
    assert set().union(*[reached_cells(c) for c in CASES]) == set(CELLS)
    for k in KINDS:     # every kind at every S, every gather
        assert {S for S in ab.SS for c in CASES if f"{k} S={S}" in reached_cells(c, (k,))} == set(ab.SS)
    for c in CASES:     # small, off the ring and LDS forward kernels, rows past the batch in every plan
        assert c.batch <= 671 and max(c.dims) <= 65 and c.max_batch > c.batch and c.e0 >= 1, c.name
        assert all(f.kernel == "k_dense_fwd" for f in dc.expected_launches(c.dense).fwd), c.name
        for kind in KINDS:
            for k in range(ab.N_STEPS):
                h = ab.bsam_hyper(c, k) if kind == "bsam" else ab.adam_hyper(c, kind, k)
                assert 0.0 <= h["beta_1"] < 1.0 and 0.0 <= h["beta_2"] < 1.0 and h["lr"] > 0, (c.name, kind, k)   # what the entry points take
                assert kind == "adam" or h["num_data"] > 0
    assert sum(c.aligned for c in CASES if c.fused) >= 1 and sum(c.aligned for c in CASES if not c.fused) >= 1
    assert set(ab.ONE_LAYER) == {"f_s4_self_l1", "u_d99", "u_d165_mse", "u_g16_plain", "u_g16_self"}


def test_step_hyper_parameters_are_what_the_table_says():
    """One step at the driver's values, one with a small beta_2, one with decay and another denom_eps; epochs differ."""
    for c in CASES:
        hs = [ab.adam_hyper(c, "adam", k) for k in range(3)]
        assert (hs[0]["lr"], hs[0]["beta_1"], hs[0]["beta_2"], hs[0]["denom_eps"], hs[0]["decay"]) == (0.01, 0.9, 0.999, 1e-3, 0.0)
        assert hs[1]["beta_2"] == (0.0 if c.L == 1 else 0.5)
        assert hs[2]["decay"] != 0.0 and hs[2]["denom_eps"] != 1e-3
        assert len({h["epoch"] for h in hs}) == 3 and min(h["epoch"] for h in hs) >= 1
        for k in range(3):
            h = ab.adam_hyper(c, "vadam", k)
            assert h["decay"] == h["denom_eps"] == h["lam"] / h["num_data"] and h["decay"] not in (0.0, 1e-3)
        bs = [ab.bsam_hyper(c, k) for k in range(3)]
        assert {q: bs[0][q] for q in bc.SETTINGS["driver"]} == bc.SETTINGS["driver"]
        assert {q: bs[1][q] for q in bc.SETTINGS["sharp"]} == bc.SETTINGS["sharp"]
        assert len({ab.philox_step(c, k) for k in range(3)}) == 3


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_data_properties(case):
    a = ab_data(case)
    D, spec = case.D, case.spec
    for v in (a.theta0, a.m0, a.v0_adam, a.v0_bsam):
        assert v.shape == (D,) and v.dtype == np.float32 and np.all(np.isfinite(v))
    assert len(a.rows) == case.batch and (a.idx is not None) == case.gathered
    assert np.all(a.m0 != 0) and np.all(a.v0_adam > 0) and a.v0_bsam.min() >= 0.5 and a.v0_bsam.max() <= 2.0
    _, g, s = ac.grad_moments(a.theta0, a.rows, a.ys, spec)
    for name, sl in ab.blocks(spec):
        assert 0.1 * np.abs(g[sl]).max() <= np.abs(a.m0[sl]).max() <= 3.0 * max(np.abs(g[sl]).max(), 1e-3 * np.abs(g).max()), name
        top = max(s[sl].max(), 1e-6 * s.max())
        assert 0.4 * ab.V0_FLOOR * top <= a.v0_adam[sl].min() and a.v0_adam[sl].max() <= 1.6 * top, name
    if case.batch == 1:
        assert np.array_equal(s, g * g)


# ---------------------------------------------------------------- the restated steps against AdamRef / BsamRef
@pytest.mark.parametrize("name", ["f_s2_odd", "f_s16_l3_mse", "u_d165_mse", "u_d218_self", "f_b1", "f_tiles_2x3"])
def test_restated_steps_equal_adamref_and_bsamref(name):
    case = ab.CASE_BY_NAME[name]
    data, spec = ab_data(case), case.spec
    same = lambda u, v: np.array_equal(np.asarray(u), np.asarray(v)) and np.asarray(u).dtype == np.asarray(v).dtype
    for k in range(ab.N_STEPS):
        s0 = ab.initial_state("adam", data)
        h = ab.adam_hyper(case, "adam", k)
        r = ac.AdamRef(s0["theta"])
        r.m, r.v = s0["m"].astype(np.float64), s0["v"].astype(np.float64)
        loss = r.step(data.rows, data.ys, spec, h["lr"], h["beta_1"], h["beta_2"], h["epoch"], h["denom_eps"], h["decay"])
        out = ref_step(case, "adam", s0, k)
        assert same(out["theta"], r.theta) and same(out["m"], r.m) and same(out["v"], r.v) and out["loss"][0] == loss

        h = ab.adam_hyper(case, "vadam", k)
        eps = ab.injected_noise(case, "vadam", "injected", k)
        r = ac.AdamRef(s0["theta"])
        r.m, r.v = s0["m"].astype(np.float64), s0["v"].astype(np.float64)
        r.perturb(eps.astype(np.float64), h["lam"], h["num_data"])
        pert = r.theta.copy()
        loss = r.step(data.rows, data.ys, spec, h["lr"], h["beta_1"], h["beta_2"], h["epoch"], h["denom_eps"], h["decay"])
        out = ref_step(case, "vadam", s0, k, variant="injected")
        assert same(out["pert"], pert) and same(out["theta"], r.theta) and same(out["m"], r.m) and same(out["v"], r.v)
        assert out["loss"][0] == loss
        again = ref_step(case, "vadam", s0, k, variant="injected", pert=pert)
        assert same(again["theta"], r.theta)

        for dtype in (np.float64, np.float32):
            s0 = ab.initial_state("bsam", data)
            eps = ab.injected_noise(case, "bsam", "injected", k)
            r = bc.BsamRef(s0["theta"], dtype)
            r.m, r.v = s0["m"].astype(dtype), s0["v"].astype(dtype)
            l1, l2 = r.step(data.rows, data.ys, spec, eps, **ab.bsam_hyper(case, k))
            out = ref_step(case, "bsam", s0, k, dtype, variant="injected")
            assert same(out["theta"], r.theta) and same(out["m"], r.m) and same(out["v"], r.v)
            assert out["theta"].dtype == dtype and tuple(out["loss"]) == (dtype(l1), dtype(l2))


def test_identity_restated_in_a_dtype_equals_adam_checks():
    for name in ("f_s16_l3_mse", "u_d99", "f_tiles_2x3"):
        case = ab.CASE_BY_NAME[name]
        d = ab_data(case)
        g, s = ab.identity_moments(d.theta0, d.rows, d.ys, case.spec)
        g0, s0 = ac.identity_moments(d.theta0, d.rows, d.ys, case.spec)
        assert np.array_equal(g, g0) and np.array_equal(s, s0)
        g32, s32 = ab.identity_moments(d.theta0, d.rows, d.ys, case.spec, np.float32)
        assert g32.dtype == s32.dtype == np.float32


def test_elementwise_tolerance_is_the_measured_one():
    """The float32 identity against the float64 per-row moments, element by element of s, on the one-layer cases' own
    inputs: the measurement behind V_ELEMENTWISE_TOL (its margin of 4 covers the kernel's other summation order)."""
    worst = 0.0
    for name in ab.ONE_LAYER:
        case = ab.CASE_BY_NAME[name]
        d = ab_data(case)
        _, _, s = ac.grad_moments(d.theta0, d.rows, d.ys, case.spec)
        _, s32 = ab.identity_moments(d.theta0, d.rows, d.ys, case.spec, np.float32)
        assert np.all(s > 0)
        rel = float((np.abs(s32.astype(np.float64) - s) / s).max())
        print(f"ELEMENTWISE | {name} | float32 identity against float64 per-row s: {rel:.3e}")
        worst = max(worst, rel)
    assert 0.5 * ab.V_ELEMENTWISE_MEASURED <= worst <= ab.V_ELEMENTWISE_MEASURED, worst
    assert ab.V_ELEMENTWISE_TOL == MARGIN * ab.V_ELEMENTWISE_MEASURED


# ---------------------------------------------------------------- the comparison: float32 passes, wrong restatements fail
def rounding_share(case, kind, base, ref):
    """Largest share of a block's update tolerance that the allowance for the stored roundings takes."""
    a0, a1 = np.asarray(base, dtype=np.float64), np.asarray(ref["theta"], dtype=np.float64)
    inc = a1 - a0
    floor = 1e-3 * np.abs(inc).max()
    worst = 0.0
    for _, sl in ab.blocks(case.spec):
        allow = ab.UPDATE_ROUNDINGS[kind] * 2.0 ** -24 * max(np.abs(a0[sl]).max(), np.abs(a1[sl]).max())
        worst = max(worst, allow / (ab.REL * max(np.abs(inc[sl]).max(), floor) + allow))
    return worst


def chain(case, kind, variant):
    """The three steps as on the device: the float32 stand-in's stored state starts the next step, and the float64
    reference restarts from it.  Returns [(s0, got, ref)]."""
    s0 = ab.initial_state(kind, ab_data(case))
    out = []
    for k in range(ab.N_STEPS):
        got = ab.as_stored(ref_step(case, kind, s0, k, np.float32, variant=variant))
        ref = ref_step(case, kind, s0, k, variant=variant, pert=got.get("pert"))
        out.append((s0, got, ref))
        s0 = {q: got[q] for q in s0}
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_comparison_passes_the_float32_restatement_and_fails_every_wrong_one(case, kind):
    for variant in CPU_VARIANTS[kind]:
        steps = chain(case, kind, variant)
        worst, shares = {}, []
        for k, (s0, got, ref) in enumerate(steps):
            rep = compare_step(case, kind, k, s0, got, ref, what=f"float32 restatement, {variant}: ")
            for q, r in rep.items():
                worst[q] = max(worst.get(q, 0.0), r)
            shares.append(rounding_share(case, kind, got["pert"] if kind == "vadam" else s0["theta"], ref))
            if variant == "device":
                bm = ab.box_muller_share(case, kind, k, s0, ref)
                print(f"BOX-MULLER | {case.name} | {kind} | step {k} | share of the tolerance {bm:.3f}")
                assert bm <= 0.5, f"{case.name} {kind} step {k}: the Box-Muller difference may take {bm:.2f} of a block's tolerance"
        # the update stands clear of the rounding of the stored weights: in every step the larger part of every block's
        # tolerance is the 1e-4 of its scale (the steps at the drivers' small learning rates come closest), in one step
        # at least three quarters
        assert max(shares) <= 0.6 and min(shares) <= 0.25, f"{case.name} {kind}: the rounding allowance takes {shares} of a block's tolerance"
        for q, r in sorted(worst.items()):     # (the table of the pull request: run with -s)
            print(f"FLOAT32 | {case.name} | {kind} | {variant} | {q} | error / tolerance {r:.4f}")
            assert r * MARGIN <= 1.0, f"{case.name} {kind} {variant}: {q}: the float32 restatement takes {r:.3f} of the tolerance"
        for mutation in MUTATIONS:
            if not ab.mutation_applies(case, kind, mutation):
                continue
            caught = False
            for k, (s0, _, ref) in enumerate(steps):
                got = ab.as_stored(ref_step(case, kind, s0, k, np.float32, mutation=mutation, variant=variant))
                if kind == "vadam":     # the update is judged from the (wrong) perturbed weights the stand-in stored
                    ref = ref_step(case, kind, s0, k, variant=variant, pert=got["pert"])
                try:
                    compare_step(case, kind, k, s0, got, ref)
                except AssertionError:
                    caught = True
                    break
            assert caught, f"{case.name} {kind} {variant}: the comparison does not see the wrong restatement '{mutation}'"


def test_every_wrong_restatement_is_exercised():
    for mutation, kinds in MUTATIONS.items():
        n = sum(ab.mutation_applies(c, k, mutation) for c in CASES for k in kinds)
        assert n >= len(CASES) - 1, (mutation, n)
    assert len(MUTATIONS) == 18
    assert [ab.mutation_applies(ab.CASE_BY_NAME["f_b1"], "adam", m) for m in ab.S_MUT] == [False, False, True, True, True]
