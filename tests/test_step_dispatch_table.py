"""The step case table (tests/step_cases.py) against the library's source and the oracle modules, on the CPU.

The update-mode constants, which kernels each pyz_*_step launches on the fused and the unfused path and their grids are
read out of pyz_fused.h, pyz_kernels.h and pyz_api.hip; the cells the cases reach are compared with the coverage table
name by name; the restated steps are held bit-equal to oracle.sgd / swag / sgld / bbb in float64 and float32; and the
comparison the GPU matrix uses is run with the float32 oracle in place of the device (it must pass, four times inside
every bound) and with every wrong oracle (each must fail on every case it applies to)."""

import re

import numpy as np
import pytest

import dense_cases as dc
import step_cases as sc
from dense_cases import pick_waves, wgrad_steps, wgrad_tiles
from oracle import bbb as o_bbb
from oracle import mlp as o_mlp
from oracle import sgd as o_sgd
from oracle import sgld as o_sgld
from oracle import swag as o_swag
from step_cases import CASES, CELLS, MODES, MUTATIONS, compare_step, expected_step_launches, reached_cells, ref_step, step_data
from test_dense_dispatch_table import function_body, src

CPU_VARIANTS = {"sgd": ("plain",), "swag": ("plain",), "sgld": ("zeros", "philox"), "bbb": ("philox",)}
MARGIN = 4.0   # the float32 oracle stays this many times inside every bound


# ---------------------------------------------------------------- the restatement against the source
def test_update_modes_and_streams_match_the_source():
    fused, rng = src("pyz_fused.h"), src("pyz_rng.h")
    found = {name.lower(): int(v) for name, v in re.findall(r"#define PYZ_UPD_(\w+) (\d+)", fused)}
    assert found == sc.UPD_MODE
    from bayesian_inference_for_nn_amd import _lib
    for mode, const in (("sgld", "PYZ_STREAM_SGLD"), ("bbb", "PYZ_STREAM_BBB")):
        m = re.search(r"#define\s+%s\s+(\d+)u?" % const, rng) or re.search(r"%s\s*=\s*(\d+)" % const, rng)
        assert m, const
        assert int(m.group(1)) == sc.STREAM[mode] == getattr(_lib, const[4:])


def test_step_functions_launch_what_the_table_says():
    api, ker = src("pyz_api.hip"), src("pyz_kernels.h")
    sgd = function_body(api, "int pyz_sgd_step(")
    assert "const bool fused = can_fuse(m);" in sgd and "u.mode = PYZ_UPD_SGD;" in sgd and "u.mode = PYZ_UPD_NONE;" in sgd
    assert "if (!fused)\n    PYZ_LAUNCH(k_sgd_update, dim3(cdiv(m->D, 256)), dim3(256), 0, st," in sgd
    swag = function_body(api, "int pyz_swag_step(")
    assert "const bool fused = can_fuse(m);" in swag and "u.mode = PYZ_UPD_SWAG;" in swag and "u.mode = PYZ_UPD_NONE;" in swag
    assert "u.dev_row = d_dev_row;" in swag and "u.swag_update = update_moments ? 1 : 0;" in swag
    assert "if (!fused)\n    PYZ_LAUNCH(k_swag_update, dim3(cdiv(m->D, 256)), dim3(256), 0, st," in swag
    step = function_body(api, "int pyz_sgld_step(")
    assert "launch_sgld_step(m, d_theta, d_mean, d_sq_mean, d_x, d_y, d_row_idx, batch, 0, false, 0, seed, d_unit_noise, d_loss, st);" in step
    sgld = function_body(api, "static void launch_sgld_step(")
    assert "int mode = PYZ_UPD_SGLD," in sgld and "if (can_fuse(m)) {" in sgld and "u.mode = mode;" in sgld
    assert sgld.index("if (can_fuse(m)) {") < sgld.index("u.mode = PYZ_UPD_NONE;") < sgld.index("PYZ_LAUNCH(k_sgld_update")
    assert "PYZ_LAUNCH(k_sgld_update, dim3(cdiv(cdiv(m->D, 4), 256)), dim3(256), 0, st, a);" in sgld
    bbb = function_body(api, "int pyz_bbb_step(")
    assert "const int nblk_kl = cdiv(cdiv(m->D, 4), 256);" in bbb
    assert bbb.index("PYZ_LAUNCH(k_bbb_sample, dim3(nblk_kl), dim3(256), 0, st, a);") < bbb.index("if (can_fuse(m)) {")
    assert bbb.index("u.mode = PYZ_UPD_BBB;") < bbb.index("} else {") < bbb.index("PYZ_LAUNCH(k_bbb_update, dim3(nblk_kl), dim3(256), 0, st, a);")
    assert bbb.count("PYZ_LAUNCH(k_bbb_sample") == 1 and bbb.count("PYZ_LAUNCH(k_bbb_update") == 1
    for fn in (sgd, swag, sgld, bbb):     # both paths go through the one gradient call whose arms the Dense table holds
        assert "launch_loss_backward(m, " in fn
    # one or four elements per thread
    for k, per in sc.PER_THREAD.items():
        body = function_body(ker, f"__global__ void {k}(")
        assert ("const long long e0 = 4 * t;" in body) == (per == 4), k
        assert ("const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;" in body) == (per == 1), k
    assert [sc.update_grid("k_sgd_update", D) for D in (1, 256, 257)] == [1, 1, 2]
    assert [sc.update_grid("k_bbb_sample", D) for D in (1, 1024, 1025, 2596)] == [1, 1, 2, 3]
    assert "(reinterpret_cast<uintptr_t>(g.w) & 15) == 0" in function_body(ker, "__global__ void k_bbb_sample(")


def test_every_kernel_that_finalises_a_loss_notes_it():
    """include/pyz.h: every kernel that finalises a step's loss counts NaN / Inf results for pyz_check_finite."""
    api, ker, fused = src("pyz_api.hip"), src("pyz_kernels.h"), src("pyz_fused.h")
    for k in ("k_sgd_update", "k_swag_update", "k_sgld_update", "k_bbb_update", "k_adam_update", "k_loss_finalize"):
        assert "pyz_note_loss(" in function_body(ker, f"__global__ void {k}("), k
    assert "pyz_note_loss(g.nonfinite, g.cost[0]);" in function_body(ker, "__global__ void k_bbb_update(")
    assert function_body(fused, "void pyz_step_duties(").count("pyz_note_loss(g.nonfinite, ") == 2
    assert "a.nonfinite = m->nonfinite;" in function_body(api, "int pyz_bbb_step(")
    assert "a.nonfinite = m->nonfinite;" in function_body(api, "int wgrad_layers(")


def test_fused_arms_follow_the_dense_table():
    for c in CASES:
        for mode in MODES:
            la = expected_step_launches(c, mode)
            assert la.sample == (mode == "bbb")
            if not c.fused:
                assert la.update == (sc.UPDATE_KERNEL[mode],) and la.S == 0 and c.dims[-1] > dc.FUSE_MAX_N
                continue
            tiles = sum(wgrad_tiles(K, N) for K, N in zip(c.dims[:-1], c.dims[1:]))
            S, _ = pick_waves(tiles, wgrad_steps(c.batch))
            assert la.S == S and S in dc.WGRAD_ALL_S and la.wgrad == (dc.wgrad_all_expr(S, False),) and la.update == ()
    by = lambda name, mode="sgd": expected_step_launches(sc.CASE_BY_NAME[name], mode)
    assert by("f_s1").wgrad == ("k_wgrad_all<1>",) and by("f_s16_l3_mse").wgrad == ("k_wgrad_all<16>",)
    assert by("f_s4_copy").gather == "copy" and by("f_s4_self_l1").gather == "self" and by("u_d218_self").gather == "self"
    assert by("u_d99", "bbb") == sc.StepLaunches(1, ("k_dense_bwd_weight",), ("k_bbb_update",), 0, "none")


# ---------------------------------------------------------------- the cases against the table
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_cell_is_reached(cell):
    assert any(cell in reached_cells(c) for c in CASES), f"no case reaches the cell '{cell}'"


def test_table_and_cases_are_complete():
    assert len(CELLS) == 58 and len(CASES) == 13
    assert set().union(*[reached_cells(c) for c in CASES]) == set(CELLS)
    for S in sc.SS:     # every S by at least two modes; every mode at S = 1, S = 16 and in between
        assert sum(any(f"{m} S={S}" in reached_cells(c, (m,)) for c in CASES) for m in MODES) >= 2
    for m in MODES:
        got = {S for S in sc.SS for c in CASES if f"{m} S={S}" in reached_cells(c, (m,))}
        assert {1, 16} <= got and got & {2, 4, 8}
    for c in CASES:     # small, off the ring and LDS forward kernels, scalars that float32 holds exactly
        assert c.batch <= 301 and max(c.dims) <= 40 and c.n0 >= 3, c.name
        assert all(f.kernel == "k_dense_fwd" for f in dc.expected_launches(c.dense).fwd), c.name
        for v in (c.lr, c.bbb_lr, c.alpha) + c.prior:
            assert float(np.float32(v)) == v, (c.name, v)
    assert sum(c.aligned for c in CASES if c.fused) >= 1 and sum(c.aligned for c in CASES if not c.fused) >= 1
    aligned_unfused = [c for c in CASES if c.aligned and not c.fused]
    assert all(c.D >= 4 for c in aligned_unfused)       # reaches the 16-byte store of k_bbb_sample


def test_cells_the_older_step_tests_reach():
    """What tests/test_gpu_parity.py (and the one sgd case of the Dense matrix) reach of this table, from their shapes: SGLD
    and SWAG at S = 1 and 8, BBB at 1, 2 and 8, SGD at 1 and 4; no S = 16, no update on a copied gather, every unfused D a
    multiple of four, every buffer a fresh aligned allocation."""
    old = {name: reached_cells(c, modes) for name, (c, modes) in sc.old_parity_shapes().items()}
    reached = set().union(*old.values())
    at = lambda m: sorted(int(c.split("=")[1]) for c in reached if c.startswith(f"{m} S="))
    assert (at("sgld"), at("swag"), at("bbb"), at("sgd")) == ([1, 8], [1, 8], [1, 2, 8], [1, 4])
    assert not any("gather=copy" in c for c in reached) and {c for c in reached if "gather=self" in c} == {"sgd gather=self"}
    assert {c[-1] for c in reached if " D%4=" in c} == {"0"}
    assert "state buffers 4 bytes off 16-byte alignment" not in reached and "K + 1 = 32" not in reached and "K + 1 = 33" not in reached
    assert len(CELLS - reached) >= 33


def blocks(spec):
    for l, ((ko, bo), K, N) in enumerate(zip(spec.offsets(), spec.dims[:-1], spec.dims[1:])):
        yield f"W{l}", slice(ko, ko + K * N)
        yield f"b{l}", slice(bo, bo + N)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_data_properties(case):
    a, b = step_data(case), step_data(case)
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v)
    D, spec = case.D, case.spec
    for v in (a.theta0, a.mean0, a.sq0, a.rho0):
        assert v.shape == (D,) and v.dtype == np.float32 and np.all(np.isfinite(v))
    assert a.dev0.shape == (2, D) and np.all(a.dev0 != 0)
    scale = np.abs(a.theta0).max()
    assert 0 < np.abs(a.mean0 - a.theta0).max() <= 0.5 * scale and np.all(a.mean0 != 0)
    assert np.all(a.sq0 >= a.mean0 * a.mean0) and np.all(a.sq0.astype(np.float64) > a.mean0.astype(np.float64) ** 2)
    assert a.rho0.min() >= -3.0 and a.rho0.max() <= 1.0 and a.rho0.min() < -2.5 and a.rho0.max() > 0.5
    assert (a.pm_vec is not None) == case.prior_vec == (a.pr_vec is not None)
    assert len(a.rows) == case.batch and (a.idx is not None) == case.gathered
    # the gradient term stands clear of the rounding of the stored parameters in every block
    _, g, _ = o_mlp.loss_and_grad(a.theta0, a.rows, a.ys, spec)
    for name, sl in blocks(spec):
        share = case.lr * np.abs(g[sl]).max() / scale
        assert share >= 5e-3, f"{case.name}: block {name}: lr max|g| is only {share:.2e} of max|theta0|"


# ---------------------------------------------------------------- the restated steps against the oracle modules
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", ["f_s2_odd", "f_s16_l3_mse", "u_d165_mse", "u_d218_self"])
def test_restated_steps_equal_the_oracle_modules(name, dtype):
    case = sc.CASE_BY_NAME[name]
    data, spec, n = step_data(case), case.spec, case.n0
    same = lambda u, v: np.array_equal(np.asarray(u), np.asarray(v)) and np.asarray(u).dtype == np.asarray(v).dtype == dtype
    s0 = sc.initial_state("sgd", data)
    st = o_sgd.SGDState(s0["theta"], dtype)
    loss, _ = o_sgd.sgd_step(st, data.rows, data.ys, spec, case.lr)
    out = ref_step(case, data, "sgd", "plain", 0, s0, dtype)
    assert same(out["theta"], st.theta) and same(out["loss"], loss)

    s0 = sc.initial_state("sgld", data)
    z = sc.injected_noise(case, "sgld", "philox", 0)
    st = o_sgld.SGLDState(s0["theta"], dtype)
    st.mean, st.sq_mean, st.n = s0["mean"].astype(dtype), s0["sq"].astype(dtype), n
    loss, _ = o_sgld.sgld_step(st, data.rows, data.ys, spec, case.lr, z)
    out = ref_step(case, data, "sgld", "philox", 0, s0, dtype)
    assert same(out["theta"], st.theta) and same(out["mean"], st.mean) and same(out["sq"], st.sq_mean) and same(out["loss"], loss)

    s0 = sc.initial_state("swag", data)
    for k, (update, row) in enumerate(sc.SWAG_STEPS):
        st = o_swag.SWAGState(s0["theta"], 2, dtype)
        st.mean, st.sq_mean, st.n = s0["mean"].astype(dtype), s0["sq"].astype(dtype), n + k
        loss = o_swag.swag_step(st, data.rows, data.ys, spec, case.lr, frequency=1 if update else n + k + 1)
        out = ref_step(case, data, "swag", "plain", k, s0, dtype)
        assert same(out["theta"], st.theta) and same(out["mean"], st.mean) and same(out["sq"], st.sq_mean) and same(out["loss"], loss)
        assert st.dev.shape[0] == int(update)
        if row is not None and update:
            assert same(out["dev"][row], st.dev[0]) and same(out["dev"][1 - row], s0["dev"][1 - row].astype(dtype))
        else:
            assert same(out["dev"], s0["dev"].astype(dtype))

    s0 = sc.initial_state("bbb", data)
    eps = sc.injected_noise(case, "bbb", "philox", 1)
    pm, pr = (data.pm_vec, data.pr_vec) if case.prior_vec else case.prior
    ref = o_bbb.bbb_step(s0["mu"], s0["rho"], eps, data.rows, data.ys, spec, case.bbb_lr, case.alpha, pm, pr, dtype)
    out = ref_step(case, data, "bbb", "philox", 1, s0, dtype)
    assert same(out["mu"], ref["mu"]) and same(out["rho"], ref["rho"]) and same(out["w"], ref["w"])
    assert same(out["cost"], np.array([ref["cost"], ref["loss"], ref["kl"]]))


# ---------------------------------------------------------------- the comparison: float32 oracle passes, wrong oracles fail
def rounding_share(case, mode, s0, ref):
    """Largest share of a block's increment tolerance that the allowance for the stored roundings takes."""
    worst = 0.0
    for key in (("mu", "rho") if mode == "bbb" else ("theta",)):
        a0, a1 = s0[key].astype(np.float64), np.asarray(ref[key], dtype=np.float64)
        inc = a1 - a0
        floor = 1e-3 * np.abs(inc).max()
        for _, sl in blocks(case.spec):
            allow = 2.0 ** -23 * max(np.abs(a0[sl]).max(), np.abs(a1[sl]).max())
            worst = max(worst, allow / (1e-4 * max(np.abs(inc[sl]).max(), floor) + allow))
    return worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_comparison_passes_the_float32_oracle_and_fails_every_wrong_oracle(case, mode):
    data = step_data(case)
    for variant in CPU_VARIANTS[mode]:
        s0 = sc.initial_state(mode, data)
        states, worst = [], {}
        for k in range(sc.N_STEPS):      # as on the device: the reference restarts from the stored state of every step
            ref = ref_step(case, data, mode, variant, k, s0)
            got = sc.as_stored(ref_step(case, data, mode, variant, k, s0, np.float32))
            rep = compare_step(case, mode, k, s0, got, ref, what=f"float32 oracle, {variant}: ")
            for q, r in rep.items():
                worst[q] = max(worst.get(q, 0.0), r)
            share = rounding_share(case, mode, s0, ref)
            assert share <= 0.25, f"{case.name} {mode} step {k}: the rounding allowance is {share:.2f} of a block's tolerance"
            states.append(s0)
            s0 = {key: got[key] for key in s0}
        for q, r in sorted(worst.items()):     # (the table of the pull request: run with -s)
            print(f"FLOAT32 | {case.name} | {mode} | {variant} | {q} | error / tolerance {r:.4f}")
            assert r * MARGIN <= 1.0, f"{case.name} {mode} {variant}: {q}: the float32 oracle takes {r:.3f} of the tolerance"
        for mutation in MUTATIONS:
            if not sc.mutation_applies(case, mode, variant, mutation):
                continue
            caught = False
            for k, s in enumerate(states):
                ref = ref_step(case, data, mode, variant, k, s)
                got = sc.as_stored(ref_step(case, data, mode, variant, k, s, np.float32, mutation=mutation))
                try:
                    compare_step(case, mode, k, s, got, ref)
                except AssertionError:
                    caught = True
                    break
            assert caught, f"{case.name} {mode} {variant}: the comparison does not see the wrong oracle '{mutation}'"


def test_every_wrong_oracle_is_exercised():
    for mutation, modes in MUTATIONS.items():
        n = sum(sc.mutation_applies(c, m, v, mutation) for c in CASES for m in modes for v in CPU_VARIANTS[m])
        assert n >= (4 if mutation == "BBB prior vector ignored" else len(CASES)), (mutation, n)
    assert len(MUTATIONS) == 12
