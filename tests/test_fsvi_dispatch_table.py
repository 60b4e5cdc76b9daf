"""The FSVI case table (tests/fsvi_cases.py) against the library's source and the restatement of fsvi_checks, on the CPU.

The strides, limits and solve rules of pyz_fsvi.h and the launches of pyz_fsvi_step are read out of the source; the forward
variant and the wave counts of every case come from the Dense rules of dense_cases (pinned to pyz_gemm.h by
tests/test_dense_dispatch_table.py); the cells the cases reach are compared with the coverage table name by name; the inputs
are held to the window that keeps the GP prior matrix away from the identity; the restated step is held to
fsvi_checks.terms; and the comparison the GPU matrix uses is run with a float32 stand-in in place of the device (it must
pass four times inside every bound) and with every wrong oracle (each must fail on every step of every case it applies to).
Run with -s for the tables."""

import re

import numpy as np
import pytest

import dense_cases as dc
import fsvi_cases as fv
import fsvi_checks as fc
from fsvi_cases import CASES, CELLS, MUTATIONS, N_STEPS, case_data, compare_step, expected_fsvi_launches, reached_cells
from test_dense_dispatch_table import function_body, squash, src

MARGIN = 4.0   # the float32 stand-in stays this many times inside every bound
IDS = [c.name for c in CASES]


# ---------------------------------------------------------------- the restatement against the source
def test_limits_strides_and_solve_rules_match_the_source():
    h = src("pyz_fsvi.h")
    defines = {name: int(v) for name, v in re.findall(r"#define (PYZ_\w+) (\d+)\b", h)}
    assert defines["PYZ_FSVI_MAX_N"] == fv.MAX_N and defines["PYZ_FSVI_MAX_D"] == fv.MAX_D
    assert defines["PYZ_SPD_MAX_N"] == fv.SPD_MAX_N and defines["PYZ_SPD_LDS_N"] == fv.SPD_LDS_N
    assert defines["PYZ_SPD_THREADS"] == fv.SPD_THREADS
    assert "static inline int pyz_spd_panel(int n) { return n <= 512 ? 32 : (n <= 1024 ? 16 : 4); }" in h
    assert [fv.spd_panel(n) for n in (129, 512, 513, 1024, 1025, 2048)] == [32, 32, 16, 16, 4, 4]
    spd = function_body(h, "static inline void pyz_launch_spd(")
    assert "const int threads = n <= 32 ? 256 : PYZ_SPD_THREADS;" in spd
    assert (fv.SPD_SMALL_N, fv.SPD_SMALL_THREADS) == (32, 256) and [fv.spd_threads(n) for n in (32, 33)] == [256, 1024]
    assert "if (n <= PYZ_SPD_LDS_N) PYZ_LAUNCH(k_spd_solve_f64<true>, dim3(n_systems), dim3(threads), lds, st," in spd
    assert "else PYZ_LAUNCH(k_spd_solve_f64<false>, dim3(n_systems), dim3(threads), lds, st," in spd
    lds = function_body(h, "static inline size_t pyz_spd_lds_bytes(")
    assert "if (n <= PYZ_SPD_LDS_N) return sizeof(double) * ((size_t)3 * n + (size_t)(n | 1) * n);" in lds
    assert "return sizeof(double) * ((size_t)2 * n + (size_t)n * (pyz_spd_panel(n) + 1));" in lds
    # the largest requests: 132 KiB in LDS, 152 KiB at n = 1024; the last size of each panel width and the entry's limit
    assert fv.spd_lds_bytes(128) == 132 * 1024 and fv.spd_lds_bytes(1024) == 152 * 1024
    assert max(fv.spd_lds_bytes(n) for n in range(1, fv.SPD_MAX_N + 1)) == fv.spd_lds_bytes(1024) <= 160 * 1024
    assert "(int)pyz_spd_lds_bytes(PYZ_SPD_LDS_N)" in h and "(int)pyz_spd_lds_bytes(1024)" in h
    # the back substitution holds two columns per thread: 2 x 1024 threads cover n = 2048
    assert "const int c = tid + q * T;" in h and "for (int q = 0; q < 2; ++q)" in h and 2 * fv.SPD_THREADS >= fv.SPD_MAX_N
    # the 256 strides
    gram = function_body(h, "__global__ void __launch_bounds__(256) k_fsvi_gram(")
    assert "const long long e = (long long)blockIdx.x * 256 + threadIdx.x;" in gram and "if (e >= (long long)n * n) return;" in gram
    assert "const float *xr = xp + ((long long)i * n + r) * F, *xs = xp + ((long long)i * n + s) * F;" in gram
    assert "exp(-0.5 * d2) + (r == s ? 1e-6 : 0.0)" in gram and "for (int c = 0; c < F; ++c)" in gram
    stein = function_body(h, "__global__ void __launch_bounds__(256) k_fsvi_stein_system(")
    assert "for (int c = tid; c < D; c += 256)" in stein and "red[0] / (double)D" in stein
    delta = function_body(h, "__global__ void __launch_bounds__(256) k_fsvi_delta(")
    assert "for (int r = tid; r < g.n; r += 256)" in delta and "for (int j = tid; j <= H; j += 256)" in delta
    assert "for (long long e = tid; e < (long long)g.n * H; e += 256)" in delta
    assert "const long long row = g.row_idx ? g.row_idx[r] : r;" in delta
    assert fv.STRIDE == 256


def test_fsvi_step_launches_what_the_table_says():
    api, gemm = src("pyz_api.hip"), src("pyz_gemm.h")
    step = function_body(api, "int pyz_fsvi_step(")
    order = ["PYZ_LAUNCH(k_fsvi_inputs, dim3(cdiv((long long)k * n * F, 256)), dim3(256), 0, st, in);",
             "PYZ_LAUNCH(k_fsvi_stein_system, dim3((unsigned)D, k), dim3(256), 0, st, d_particles, (int)D, skm, srhs);",
             "pyz_launch_spd(skm, srhs, (int)D, k, fail + k, st);",
             "pyz_launch_fwd(g, n, k, st);",
             "PYZ_LAUNCH(k_fsvi_gram, dim3(cdiv((long long)n * n, 256), k), dim3(256), 0, st, xp, n, F, f,",
             "pyz_launch_spd(gram, alpha, n, k, fail, st);",
             "PYZ_LAUNCH(k_fsvi_delta, dim3(k), dim3(256), 0, st, dg);",
             "launch_bwd_data_hidden(m, d_particles, D, k, n, m->ctl, st);",
             "pyz_launch_bwd_weight(g, n, k, st);",
             "PYZ_LAUNCH(k_fsvi_update, dim3(cdiv(D, 256)), dim3(256), 0, st, u);"]
    at = [step.index(s) for s in order]
    assert at == sorted(at)
    assert "pyz_launch_fwd_ring" not in step
    # per-particle rows at layer 0 of the forward and of the weight gradient, and under the one-layer arm of k_fsvi_delta
    assert step.count("g.in_pstride = (long long)n * F;") == 2 and "dg.h_pstride = (long long)n * F;" in step
    assert "for (int ll = m->L - 2; ll >= 0; --ll)" in step
    assert "in.row_idx = d_row_idx;" in step and "dg.row_idx = d_row_idx;" in step
    assert "const int n = batch + batch_size, F = m->dims[0];" in step
    check = function_body(api, "int pyz_fsvi_check(")
    assert "(long long)batch + batch_size > PYZ_FSVI_MAX_N" in check and "D > PYZ_FSVI_MAX_D" in check
    assert "n < 1 || n > PYZ_SPD_MAX_N" in function_body(api, "int pyz_spd_solve_f64(")
    hidden = function_body(api, "void launch_bwd_data_hidden(")
    assert "for (int l = m->L - 2; l >= 1; --l)" in hidden
    # the LDS forward's rule that only per-particle input rows exercise, and the switch the `ldsfwd` case flips per call
    takes = function_body(gemm, "static inline bool pyz_fwd_takes_lds(")
    assert "(P == 1 || g.in_pstride % 4 == 0)" in takes and "(P == 1 || g.theta_pstride % 2 == 0)" in takes
    assert 'wg128 >= pyz_env_int("PYZ_FWD_LDS_MINWG", 256);' in takes and "static" not in takes.split("{", 1)[1]
    assert "g.vec = (g.K % 8 == 0) && aligned16(g.in) ? 1 : 0;" in function_body(api, "DenseArgs forward_args(")
    assert squash("const long long tiles = (long long)((g.K + 1 + 31) / 32) * ((g.N + 31) / 32);\n"
                  "  const int S = pyz_pick_waves(tiles * P, (grid_batch + 1) / 2);") in squash(
        function_body(gemm, "static inline void pyz_launch_bwd_weight("))


def test_forward_variants_and_wave_counts():
    by = {c.name: expected_fsvi_launches(c) for c in CASES}
    for c in CASES:
        la = by[c.name]
        assert len(la.sequence) == 7 + c.L + max(c.L - 2, 0) + (c.L - 1), c.name
        assert [f.S for f in la.fwd] == [dc.pick_waves(dc.fwd_tiles(c.n, N) * c.k, dc.fwd_steps(K))[0]
                                         for K, N in zip(c.dims[:-1], c.dims[1:])]
        assert all(w.S == dc.pick_waves(w.tiles * c.k, dc.wgrad_steps(c.n))[0] for w in la.wgrad)
        if c.name != "ldsfwd":
            assert all(f.kernel == "k_dense_fwd" for f in la.fwd), c.name
    lds = fv.CASE_BY_NAME["ldsfwd"]
    assert [f.kernel for f in by["ldsfwd"].fwd] == ["k_dense_fwd_lds<2>", "k_dense_fwd", "k_dense_fwd", "k_dense_fwd"]
    assert all(f.kernel == "k_dense_fwd" for f in expected_fsvi_launches(lds._replace(env={})).fwd)    # without the switch
    assert lds.D % 2 == 0 and by["ldsfwd"].fwd[0].in_pstride == 512 and by["ldsfwd"].fwd[0].S == 1
    # every two- and three-layer shape with an even first width has an odd D: (F + 1) H + H + 1 and its three-layer kin
    assert all(((F + 1) * H + H + 1) % 2 == 1 for F in (2, 4) for H in (48, 64, 128))
    assert all(((F + 1) * H + (H + 1) * H2 + H2 + 1) % 2 == 1 for F in (2, 4) for H in (48, 64) for H2 in (2, 3, 8))
    # the wave counts the cases were picked for
    assert [w.S for w in by["rows514"].wgrad] == [16] and [w.S for w in by["lds128"].wgrad] == [8]
    assert [f.S for f in by["deep"].fwd] == [1, 2, 2] and by["deep"].bwd_data == ((1, 2),)
    assert by["vec8"].fwd[0].vec == 1 and by["vec8"].fwd[0].in_pstride == 56 and by["wide1"].fwd[0].S == 16
    assert (by["rows514"].gp, by["rows514"].gp_panel) == ("k_spd_solve_f64<false>", 16)
    assert (by["glob129"].gp_panel, by["lds128"].gp_panel, by["gram2"].stein_panel) == (32, 0, 0)
    assert [by[n].stein_panel for n in ("d161", "d385", "d601", "h256", "deep")] == [32, 32, 16, 4, 4]
    for c in CASES:     # (the table of the pull request: run with -s)
        la = by[c.name]
        print(f"LAUNCHES | {c.name} | D {c.D} n {c.n} k {c.k} | stein {la.stein} panel {la.stein_panel} | gp {la.gp} panel "
              f"{la.gp_panel} | fwd " + ", ".join(f"{f.kernel} S={f.S} vec={f.vec}" for f in la.fwd) +
              " | wgrad " + (", ".join(f"l{w.layer} S={w.S} tiles={w.tiles}" for w in la.wgrad) or "-"))


# ---------------------------------------------------------------- the cases against the table
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_cell_is_reached(cell):
    assert any(cell in reached_cells(c) for c in CASES), f"no case reaches the cell '{cell}'"


def test_table_and_cases_are_complete():
    assert len(CELLS) == 32 and len(CASES) == 12
    assert set().union(*[reached_cells(c) for c in CASES]) == set(CELLS)
    for c in CASES:
        assert c.n <= fv.MAX_N and c.D <= fv.MAX_D and c.k in (2, 3) and c.dims[-1] == 1, c.name
    cells = {c.name: reached_cells(c) for c in CASES}
    assert "delta: ragged third trip of the row loop" in cells["rows514"] and "delta: a loss row r >= 256" in cells["rows514"]
    assert "delta: the bias j = H alone in the second trip" in cells["h256"]
    assert "delta: one-layer arm, second trip reads xp" in cells["wide1"] and "row_idx NULL" in cells["vec8"]
    assert "layer 0 forward: k_dense_fwd_lds on per-particle rows" in cells["ldsfwd"]
    # what tests/test_gpu_fsvi.py reaches of this table, from its shapes (widths <= 8, F = 2, D <= 105, n <= 12)
    old = [fv.FsviCase("tanh8", (2, 8, 1), ("tanh", "linear"), 3, 5, 5), fv.FsviCase("relu88", (2, 8, 8, 1), ("relu", "relu", "linear"), 3, 1, 5),
           fv.FsviCase("dense1", (2, 1), ("linear",), 1, 5, 5)]
    reached = set().union(*[reached_cells(c) for c in old])
    assert reached == {"gp solve in LDS", "stein solve in LDS", "row_idx gather", "k = 3", "b < B", "gram: ragged last workgroup",
                       "k_dense_bwd_data over k particles"}, sorted(reached)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_data_and_input_conditions(case):
    """The window of the GP prior matrix from the restated Xp of every step and particle, the Stein system's conditioning
    from the particles of both steps (the second step's: the stand-in's), and the layout of the data."""
    a, b = case_data(case), case_data(case)
    assert a is b
    data = a
    assert data.x.shape == (case.b + fv.EXTRA_ROWS, case.F) and data.x.dtype == np.float32 and data.W0.shape == (case.k, case.D)
    unused = np.ones(len(data.x), dtype=bool)
    s0 = fv.initial_state(data)
    for t in range(1, N_STEPS + 1):
        d = data.steps[t - 1]
        assert (d.idx is not None) == case.gathered
        if case.gathered:
            assert sorted(d.idx) == sorted(data.steps[0].idx) and len(set(d.idx.tolist())) == case.b
            assert not np.array_equal(d.idx, np.sort(d.idx))
            unused[d.idx] = False
        else:
            unused[:case.b] = False
        xd, _ = fv.batch_of(case, data, d)
        assert np.abs(xd).max() < fv.FAR / 10
        conds = fv.assert_input_conditions(fc.make_xp(xd, d.xm, d.z), f"{case.name} t={t}")
        sconds = [fv.stein_cond(w) for w in s0["W"]]
        assert max(sconds) <= fv.STEIN_COND_MAX, (case.name, t, sconds)
        print(f"INPUTS | {case.name} | t={t} | cond(K_i) " + " ".join(f"{c:.2f}" for c, _ in conds) + " | median row maximum " +
              " ".join(f"{m:.3f}" for _, m in conds) + " | cond(K_w + 1e-3 I) " + " ".join(f"{s:.2e}" for s in sconds))
        s0 = fv.stored(fv.standin_step(case, data, t, s0))
    assert unused.sum() == fv.EXTRA_ROWS and np.all(data.x[unused] == fv.FAR)
    assert not np.array_equal(data.steps[0].xm, data.steps[1].xm)


def test_the_older_step_tests_have_an_identity_gram():
    """tests/test_gpu_fsvi.py draws its rows in [-30, 30]^2, with its own seeds and in its own order (restated here): K_i is
    the identity but for an accidental pair of rows.  Over the 36 steps of the chained test the median over the rows of the
    largest off-diagonal entry is at most 1.2e-8 and cond(K_i) at most 1.89 (the largest single entry: 0.31 on `dense1`,
    0.068 on `tanh8`, 4.9e-3 on `relu88`; 21 of the 36 steps have none above 1e-6); the terms test has one pair at 0.57 to
    0.71 and a median of 6.5e-31.  Every one misses the window the inputs are held to here."""
    B, worst_med, worst_cond, quiet = 5, 0.0, 0.0, 0
    for name in ("dense1", "tanh8", "relu88"):
        spec = fc.specs()[name]
        for k in (1, 3):
            for b in (B, 1):
                seed = sum(map(ord, name)) + k
                x, _, _, _ = fc.make_problem(spec, 9, B, k, seed)
                rng = np.random.default_rng(seed + 100)
                for _ in (1, 2, 3):
                    idx = rng.permutation(9)[:b]
                    xm = rng.uniform(-30, 30, size=(B, 2)).astype(np.float32)
                    z = (0.1 * rng.normal(size=(k, 2))).astype(np.float32)
                    rng.normal(size=(k, spec.n_params))
                    xp = fc.make_xp(x[idx], xm, z)
                    conds = fv.input_conditions(xp)
                    worst_cond, worst_med = max([worst_cond] + [c for c, _ in conds]), max([worst_med] + [m for _, m in conds])
                    quiet += all((fc.gram(xi) - np.diag(np.diag(fc.gram(xi)))).max() < 1e-6 for xi in xp)
    print(f"OLDER STEP TESTS | worst cond(K_i) {worst_cond:.3f} | worst median row maximum {worst_med:.2e} | {quiet} of 36 steps "
          "with no off-diagonal entry above 1e-6")
    assert worst_cond < fv.COND_MIN and worst_med < 1e-6 * fv.ROWMAX_MIN and quiet >= 18
    x, _, _, _ = fc.make_problem(fc.specs()["tanh8"], 9, 6, 3, 3)          # test_terms_with_injected_draws
    rng = np.random.default_rng(103)
    xm = rng.uniform(-30, 30, size=(6, 2)).astype(np.float32)
    z = (0.1 * rng.normal(size=(3, 2))).astype(np.float32)
    assert all(med < 1e-6 * fv.ROWMAX_MIN for _, med in fv.input_conditions(fc.make_xp(x[[7, 2, 5, 0, 8, 3]], xm, z)))


# ---------------------------------------------------------------- the restated step against fsvi_checks
@pytest.mark.parametrize("name", ["gram2", "d161", "deep", "wide1"])
def test_restated_terms_equal_fsvi_checks(name):
    case = fv.CASE_BY_NAME[name]
    data = case_data(case)
    d = data.steps[0]
    xd, y = fv.batch_of(case, data, d)
    mine = fv.terms(case, data.W0, xd, y, d.xm, d.z)
    theirs = fc.terms(data.W0, xd, y, d.xm, d.z, case.spec, case.B)
    assert np.array_equal(mine["xp"], theirs["xp"]) and np.array_equal(mine["f"], theirs["f"])
    assert np.array_equal(mine["alpha"], theirs["alpha"]) and np.array_equal(mine["c2"], theirs["c2"])
    assert np.abs(mine["g"] - theirs["g"]).max() <= 1e-13 * np.abs(theirs["g"]).max()
    assert abs(mine["loss"] - theirs["loss"]) <= 1e-14 * theirs["loss"]
    wrong = fc.terms(data.W0, xd, y, d.xm, d.z, case.spec, case.B, data_scale=1.0 / (case.B * case.k))
    scaled = fv.terms(case, data.W0, xd, y, d.xm, d.z, mutation=fv.M_SCALE[0])
    assert np.abs(scaled["g"] - wrong["g"]).max() <= 1e-13 * np.abs(wrong["g"]).max()
    fresh = fv.terms(case, data.W0, xd, y, d.xm, d.z, mutation=fv.M_INPUT[2])
    assert np.array_equal(fresh["xp"], fc.make_xp(xd, d.xm, d.z, "fresh")) and not np.array_equal(fresh["xp"], mine["xp"])


# ---------------------------------------------------------------- the comparison: the stand-in passes, wrong oracles fail
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_comparison_passes_the_float32_standin_and_fails_every_wrong_oracle(case):
    data = case_data(case)
    s0 = fv.initial_state(data)
    worst, caught = {}, {m: [] for m in MUTATIONS if fv.mutation_applies(case, m)}
    for t in range(1, N_STEPS + 1):      # as on the device: the reference restarts from the stored state of every step
        ref = fv.ref_step(case, data, t, s0)
        got = fv.standin_step(case, data, t, s0)
        rep = compare_step(case, data, t, s0, got, ref, what="float32 stand-in: ")
        for q, r in rep.items():
            worst[q] = max(worst.get(q, 0.0), r)
        for mutation in caught:
            bad = fv.standin_step(case, data, t, s0, mutation)
            try:
                compare_step(case, data, t, s0, bad, ref)
            except AssertionError as e:
                caught[mutation].append(str(e).split(": ", 1)[1][:60])
        s0 = fv.stored(got)
    print(f"FLOAT32 | {case.name} | " + " | ".join(f"{q} {r:.4f}" for q, r in sorted(worst.items())))
    for q, r in worst.items():
        assert r * MARGIN <= 1.0, f"{case.name}: {q}: the float32 stand-in takes {r:.3f} of the tolerance"
    for mutation, seen in caught.items():
        print(f"CAUGHT | {case.name} | {mutation} | " + " ; ".join(seen))
        assert len(seen) == N_STEPS, f"{case.name}: the comparison does not see the wrong oracle '{mutation}' on every step: {seen}"


def test_every_wrong_oracle_is_exercised():
    n = {m: sum(fv.mutation_applies(c, m) for c in CASES) for m in MUTATIONS}
    assert len(MUTATIONS) == 14 and min(n.values()) >= 1, n
    assert n[fv.M_DELTA[0]] == 1 and n[fv.M_DELTA[1]] == 1 and n[fv.M_DELTA[2]] == 2 and n[fv.M_STEIN[0]] == 6
    for m in fv.M_GRAM + fv.M_STEIN[1:] + (fv.M_INPUT[0], fv.M_INPUT[2]) + fv.M_SCALE:
        assert n[m] == len(CASES), (m, n[m])
    assert n[fv.M_INPUT[1]] == len(CASES) - 1      # (a one-layer model has no layer below the last)
