"""The run case table (tests/run_cases.py) against the library's source and the oracle modules, on the CPU.

The host rules of sgld_run_impl, of the table upload it shares with the other run entries (upload_run_tables) and of the
graph cache (PyzGraphCache) restated in run_cases (table transport, batch-ahead, first-batch launch, graph chunks, the
partition of pyz_prep_rows, the chain rules of pyz_prepare_next, the SWAG row, the BBB gate) are pinned to the text of
pyz_api.hip, pyz_fused.h, pyz_kernels.h and pyz_common.h; the cells the cases and bookkeeping runs reach are compared with
the coverage table name by name; pyz_prep_rows' restatement must hand every row of every batch size to exactly one worker;
the run reference (a chain of step_cases.ref_step) is held bit-equal to oracle.sgd / swag / sgld / bbb over a whole short
run in float64; and the comparison the GPU matrix uses is run with the float32 run reference in place of the device (it
must pass) and with every wrong run reference (each must fail on every case it applies to)."""

import os
import re

import numpy as np
import pytest

import run_cases as rc
import step_cases as sc
from dense_cases import cdiv
from oracle import bbb as o_bbb
from oracle import philox as o_philox
from oracle import sgd as o_sgd
from oracle import sgld as o_sgld
from oracle import swag as o_swag
from run_cases import BOOKS, CASES, CELLS, MODES, RUN_MUTATIONS, compare_run_step, ref_run_step, run_data
from test_dense_dispatch_table import CSRC, env_default, function_body, squash, src

_DATA = {}


def data_of(case):
    if case.name not in _DATA:
        _DATA[case.name] = run_data(case)
    return _DATA[case.name]


# ---------------------------------------------------------------- the restated rules against the source
def test_constants_and_conditions_match_the_source():
    api, ker, fused, common = src("pyz_api.hip"), src("pyz_kernels.h"), src("pyz_fused.h"), src("pyz_common.h")
    assert int(re.search(r"#define PYZ_INLINE_TAB (\d+)", ker).group(1)) == rc.INLINE_TAB
    assert int(re.search(r"#define PYZ_GRAPH_CHUNKS (\d+)", common).group(1)) == rc.GRAPH_CHUNKS
    assert env_default(api, "PYZ_GRAPH_STEPS") == rc.GRAPH_STEPS
    assert env_default(api, "PYZ_BATCH_AHEAD") == 1 and env_default(api, "PYZ_BBB_FUSE_SAMPLE") == 1
    assert env_default(api, "PYZ_FWD_KSPLIT") == 0
    for name in ("PYZ_GRAPH_STEPS", "PYZ_BATCH_AHEAD", "PYZ_BBB_FUSE_SAMPLE"):      # read once per process
        assert re.search(r'static const int \w+ =[^;]*pyz_env_int\("%s"' % name, api), name
    assert set(rc.ENV_FORBIDDEN) >= {"PYZ_GRAPH_STEPS", "PYZ_BATCH_AHEAD", "PYZ_BBB_FUSE_SAMPLE", "PYZ_FWD_KSPLIT"}
    run = function_body(api, "static int sgld_run_impl(")
    up = function_body(api, "static int upload_run_tables(")
    cache = function_body(common, "struct PyzGraphCache {")
    # table transport and the first batch: the upload every run entry shares, asked by sgld_run_impl for its largest batch
    assert "if ((rc = upload_run_tables(m, h_batch_sizes, h_lr, n_steps, n0, slot0, nullptr, d_x, d_row_idx,\n" \
           "                              batch_ahead(m, d_row_idx) ? bmax : 0, st)))" in run
    assert "if (n_steps <= PYZ_INLINE_TAB) {" in up
    inline, pinned = up[up.index("if (n_steps <= PYZ_INLINE_TAB) {"):].split("\n    return PYZ_OK;\n  }\n", 1)
    assert inline.index("if (ahead_batch) {") < inline.index("const PrepArgs pa = prep_args(m, d_x, d_row_idx, ahead_batch, row_stride, 0);") \
        < inline.index("PYZ_LAUNCH(k_run_start, dim3(256), dim3(256)") < inline.index("\n    } else {\n") \
        < inline.index("PYZ_LAUNCH(k_set_ctl_tabs, dim3(1), dim3(64)")
    assert "m->tab_bs, m->tab_lr, (long long)n0, slot0 * row_stride, (int)slot0, pa);" in inline and "k_prep_batch" not in inline
    assert "set_ctl(m, 0, h_batch_sizes[0], h_lr[0], n0, slot0 * row_stride, 0, st, (int)slot0, n_steps)" in pinned
    assert pinned.index("set_ctl(m, 0, h_batch_sizes[0]") < pinned.index("  if (ahead_batch)   //") < pinned.index("PYZ_LAUNCH(k_prep_batch,")
    assert "PYZ_LAUNCH(k_prep_batch, dim3(256), dim3(256), 0, st, prep_args(m, d_x, d_row_idx, ahead_batch, row_stride, 0), m->ctl);" in pinned
    assert "const long long row_stride = m->max_batch;" in run and "const long long row_stride = m->max_batch;" in up
    # the padding entry repeats the last step's
    assert "tabs.bs[n_steps] = h_batch_sizes[n_steps - 1];" in inline and "hb[n_steps] = h_batch_sizes[n_steps - 1];" in pinned
    assert "tabs.lr[n_steps] = h_lr[n_steps - 1];" in inline and "hl[n_steps] = h_lr[n_steps - 1];" in pinned
    # graphs: chunks of G in slot 0, the remainder by exact length in slots 1 .., a free slot before the least recently used one
    assert 'static const int G = std::min(128, std::max(2, pyz_env_int("PYZ_GRAPH_STEPS", 32) & ~1));' in run
    assert "if (use_graph && st != nullptr && !pyz_probe().on) {" in run
    assert "const int len = std::min(G, n_steps - s);" in run and "const bool rest = len < G;" in run
    assert "rc = m->graphs.launch(len, 0, rest ? 1 : 0, rest ? PYZ_GRAPH_CHUNKS : 1, st, [&] {" in run
    assert "PyzGraphCache<PYZ_GRAPH_CHUNKS> graphs;" in function_body(common, "struct pyz_mlp {")
    assert "for (int c = lo; c < hi; ++c) {\n      if (!exec[c]) {\n        if (free_slot < 0) free_slot = c;\n        continue;\n      }\n" in cache
    assert "if (len[c] == n && sig[c] == s) ci = c;" in cache
    assert "if (lru < 0 || use[c] < use[lru]) lru = c;" in cache and "ci = free_slot >= 0 ? free_slot : lru;" in cache
    assert "use[ci] = ++clock;" in cache
    # one cache type: no run entry keeps slot arrays of its own
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")):
            for old in ("ar_exec", "hr_exec", "graph_exec["):
                assert old not in src(name), (name, old)
    # every step is launched for the largest batch of the call, on StepCtl slot k & 1, the first flagged
    assert "launch_sgld_step(m, d_theta, d_mean, d_sq_mean, d_x, d_y, d_row_idx, bmax, k & 1, true, row_stride, seed,\n" \
           "                           nullptr, d_losses, st, mode, swag, bbb, k == 0);" in run
    assert "launch_sgld_step(m, d_theta, d_mean, d_sq_mean, d_x, d_y, d_row_idx, bmax, s & 1, true, row_stride, seed, nullptr,\n" \
           "                     d_losses, st, mode, swag, bbb, s == 0);" in run
    assert "if (bbb && bbb->w2 && ((n_steps - 1) & 1))" in run
    assert "if (mode != PYZ_UPD_SGLD && !can_fuse(m))" in run
    # everything baked into a graph is in its key
    for baked in ("d_theta", "d_mean", "d_sq_mean", "d_x", "d_y", "d_row_idx", "d_losses", "m->tab_bs", "swag->dev", "bbb->pm_vec",
                  "bbb->pr_vec", "bbb->val", "bbb->val_x", "bbb->val_y", "bbb->val_losses", "bbb->w2", "bbb->rho"):
        assert f"mix((unsigned long long)(uintptr_t){baked});" in run, baked
    for baked in ("mix(seed);", "mix((unsigned long long)bmax);", "mix((unsigned long long)mode);", "mix((unsigned long long)swag->k);",
                  "mix((unsigned long long)swag->freq);", "mix((unsigned long long)bbb->n_val);",
                  "memcpy(&fb[0], &bbb->alpha, 4); memcpy(&fb[1], &bbb->prior_mean, 4); memcpy(&fb[2], &bbb->prior_rho, 4);"):
        assert baked in run, baked
    # batch-ahead
    ahead = function_body(api, "inline bool batch_ahead(")
    assert "if (!on || !can_fuse(m) || m->L <= 1 || row_idx == nullptr) return false;" in ahead
    assert "return on == 2 || wgrad_tiles(m) + 24 <= pyz_cu_count();" in ahead and rc.AHEAD_SPARE == 24
    assert "if (a.prep.src && P == 1) grid.x = (unsigned)(tiles + 1 + std::max(pyz_cu_count() - tiles - 1, 24));" in api
    prep = function_body(api, "PrepArgs prep_args(")
    assert "p.fwd_tiles_n = (m->dims[1] + 31) / 32;" in prep and "p.fwd_tiles = ((grid_batch + 31) / 32) * p.fwd_tiles_n;" in prep
    # the step: BBB samples on the first step only when the sampling is fused, validates behind a gate of 10
    step = function_body(api, "static void launch_sgld_step(")
    assert "const bool sample = !fuse || first;" in step and "if (ahead) u.prep = prep_args(m, x, row_idx, grid_batch, row_stride, slot ^ 1);" in step
    assert step.count("v->ctl, st, nullptr, v->L - 1, ctl, 10);") == 1 and step.count("false, st, ctl, 10);") == 1
    assert "k_loss_finalize_gated, dim3(1), dim3(64), 0, st, v->part, v->cur_nblk, v->ctl, bbb->val_losses, v->nonfinite, ctl, 10);" in step
    assert rc.GATE_MOD == 10 and "if (gate->n % gate_mod == 0) return;" in function_body(ker, "__global__ void k_loss_finalize_gated(")
    assert "if (g.gate && g.gate->n % g.gate_mod == 0) return;" in fused and "if (g.gate && g.gate->n % g.gate_mod == 0) return;" in src("pyz_gemm.h")
    assert "a.next = chained ? m->ctl + (slot ^ 1) : nullptr;" in step and "a.loss_indexed = chained ? 1 : 0;" in step
    # the chain rules
    nxt = function_body(ker, "void pyz_prepare_next(")
    for line in ("const int i2 = ctl->i + 1;", "next->batch = tab_bs[i2];", "next->lr = tab_lr[i2];", "next->n = ctl->n + 1;",
                 "next->row_off = ctl->row_off + row_stride;", "next->slot0 = ctl->slot0;"):
        assert line in nxt, line
    duties = function_body(fused, "void pyz_step_duties(")
    assert "g.loss + (g.loss_indexed ? g.ctl->slot0 + g.ctl->i : 0);" in duties
    assert "g.cost + (g.bbb_chained ? 4 * (g.ctl->slot0 + g.ctl->i) : 0);" in duties
    math = function_body(fused, "PyzUpdOut pyz_update_math(")
    assert "const bool upd = g.swag_freq > 0 ? (nstep % g.swag_freq == 0) : (g.swag_update != 0);" in math
    assert squash("g.dev_base + min((nstep + g.swag_freq - 1) / g.swag_freq, (long long)g.swag_k - 1) * g.dev_stride") in squash(math)
    assert "const float blr = g.bbb_chained ? lr : g.bbb_lr;" in math
    assert [rc.swag_row(n, 3, 2) for n in range(7)] == [0, 1, 1, 2, 2, 2, 2] and rc.swag_row(9, 1, 3) == 0
    # the unfused loss partials
    assert "inline int loss_nblk(const pyz_mlp *m, int grid_batch) { return std::min(cdiv(m->max_batch, 256), cdiv(grid_batch, 256)); }" in api


def test_prep_rows_restatement_matches_the_source():
    fused = src("pyz_fused.h")
    body = squash(function_body(fused, "void pyz_prep_rows("))
    for line in ("if (cnt >= 8 && g.fwd_tiles >= 8) {",
                 "const int x = bid & 7, q = g.fwd_tiles >> 3, r = g.fwd_tiles & 7;",
                 "const int t0 = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q, t1 = t0 + (x < r ? q + 1 : q);",
                 "const int b0 = (t0 + g.fwd_tiles_n - 1) / g.fwd_tiles_n, b1 = (t1 + g.fwd_tiles_n - 1) / g.fwd_tiles_n;",
                 "const int r0 = min(32 * b0, nb), r1 = x == 7 ? nb : min(32 * b1, nb);",
                 "const int id0 = bid - j;", "const int first = id0 + ((x - (id0 & 7)) & 7);",
                 "const int mine = (bid - first) >> 3, all = (id0 + cnt - 1 - first) / 8 + 1;",
                 "const int per = (r1 - r0 + all - 1) / all;", "ra = r0 + mine * per;", "rb = min(ra + per, r1);",
                 "const int per = (nb + cnt - 1) / cnt;", "ra = j * per;", "rb = min(ra + per, nb);"):
        assert squash(line) in body, line
    wg = function_body(fused, "__global__ void __launch_bounds__(64 * S) k_wgrad_all(")
    assert squash("pyz_prep_rows(g.prep, g.prep.row_idx + g.ctl->row_off + g.prep.row_stride, g.prep.tab_bs[i2],\n"
                  "(int)blockIdx.x - g.tiles - 1, (int)gridDim.x - g.tiles - 1, (int)blockIdx.x);") in squash(wg)
    assert "if (i2 < g.ctl->n_run)" in wg
    for k in ("k_prep_batch", "k_run_start"):
        assert "(int)blockIdx.x, (int)gridDim.x, (int)blockIdx.x);" in function_body(fused, f"__global__ void {k}(")
    copy = function_body(fused, "void pyz_copy_rows(")
    assert "if ((K & 3) == 0 && (g.lda & 3) == 0 && ((reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst)) & 15) == 0) {" in copy


def test_prep_rows_hands_every_row_to_exactly_one_worker():
    """For every fused multi-layer case, the worker counts the launches use (256 stand-alone; max(CUs - tiles - 1, 24) in
    the epilogue, first worker id tiles + 1) and every batch size 1 .. bmax."""
    combos = 0
    for case in CASES:
        if not case.ahead:
            continue
        ft, tn = rc.fwd_tile_grid(case.dims, case.bmax)
        tiles = rc.wgrad_tile_count(case.dims)
        assert rc.epilogue_workers(case.dims) == max(rc.CUS - tiles - 1, 24)
        for cnt, first in ((rc.PREP_GRID, 0), (rc.epilogue_workers(case.dims), tiles + 1)):
            for nb in range(1, case.bmax + 1):
                parts, _ = rc.prep_partition(nb, cnt, first, ft, tn)
                owner = np.zeros(nb, dtype=np.int64)
                for ra, rb in parts:
                    assert 0 <= ra and rb <= nb, (case.name, cnt, nb, ra, rb)
                    if ra < rb:
                        owner[ra:rb] += 1
                assert np.all(owner == 1), f"{case.name}: {cnt} workers from id {first}, batch {nb}: rows {np.flatnonzero(owner != 1)[:8]}"
                combos += 1
    assert combos == 2 * sum(c.bmax for c in CASES if c.ahead)


# ---------------------------------------------------------------- the cases against the table
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_cell_is_reached(cell):
    assert any(cell in rc.reached_cells(c) for c in CASES) or any(cell in rc.book_cells(b) for b in BOOKS), \
        f"nothing reaches the cell '{cell}'"


def test_table_and_cases_are_complete():
    reached = set().union(*[rc.reached_cells(c) for c in CASES], *[rc.book_cells(b) for b in BOOKS])
    assert reached == set(CELLS)
    shape = lambda name: (CASE(name).S, rc.fwd_tile_grid(CASE(name).dims, CASE(name).bmax))
    CASE = lambda name: rc.CASE_BY_NAME[name]
    assert shape("r_s4") == (4, (2, 1)) and shape("r_s4_scalar_copy") == (4, (2, 1)) and shape("r_s2") == (2, (2, 1))
    assert shape("r_s1") == (1, (1, 1)) and shape("r_s4_xcd12") == (4, (12, 3)) and shape("r_s8_xcd8_l3_mse") == (8, (8, 2))
    assert shape("r_s16_xcd24") == (16, (24, 3)) and CASE("r_l1").S == 4 and not CASE("r_l1").ahead and CASE("r_l1").fused
    assert [c.D for c in rc.UNFUSED_CASES] == [1100, 218] and all(c.modes == ("sgld",) for c in rc.UNFUSED_CASES)
    for c in CASES:
        assert c.max_batch == c.bmax + 3 and c.sizes[0] == c.bmax == max(c.sizes) and 1 in c.sizes and c.slot0 > 0 and c.n0 > 0
        assert min(c.sizes[1:]) < c.bmax and any(b % 2 and b > 1 for b in c.sizes[1:])
        assert (c.modes == MODES) == c.fused
        for v in (c.lr, c.bbb_lr) + tuple(c.lr * f for f in rc.LR_FACTORS):
            assert float(np.float32(v)) == v
        assert len(set(zip(rc.LR_FACTORS, rc.LR_FACTORS[1:]))) == 5 and all(a != b for a, b in zip(rc.LR_FACTORS, rc.LR_FACTORS[1:]))
    for m in MODES:      # every mode at every S
        assert {c.S for c in rc.FUSED_CASES if m in c.modes} == set(sc.SS)
    assert rc.graph_chunks(32) == [32] and rc.graph_chunks(33) == [32, 1] and rc.graph_chunks(70) == [32, 32, 6] and rc.graph_chunks(5) == [5]
    assert rc.table_transport(32) == "inline" and rc.table_transport(33) == "pinned"
    assert rc.first_batch_launch((24, 16, 4), 32) == "k_run_start" and rc.first_batch_launch((24, 16, 4), 33) == "k_prep_batch"
    assert rc.first_batch_launch((31, 10), 3) is None and rc.first_batch_launch((12, 20, 40), 3) is None
    assert rc.expected_run_launches(CASE("r_s4"), "bbb", 2, n_val=rc.N_VAL) == [
        "k_set_ctl", "k_run_start", "k_bbb_sample", "k_dense_fwd", "k_head_rows<1,4,1>", "k_wgrad_all<4>", "k_dense_fwd",
        "k_head_rows<1,4,1>", "k_loss_finalize_gated", "k_dense_fwd", "k_head_rows<1,4,1>", "k_wgrad_all<4>", "k_dense_fwd",
        "k_head_rows<1,4,1>", "k_loss_finalize_gated"]
    assert rc.expected_run_launches(CASE("r_unfused_d218"), "sgld", 1) == [
        "k_set_ctl_tabs", "k_dense_fwd", "k_dense_fwd", "k_loss_scce", "k_dense_bwd_data", "k_dense_bwd_weight", "k_dense_bwd_weight",
        "k_sgld_update"]
    assert rc.expected_run_launches(CASE("r_l1"), "sgd", 33)[:4] == ["k_set_ctl", "k_head_rows<1,12,1>", "k_wgrad_all<4>", "k_head_rows<1,12,1>"]


def test_cells_the_older_run_tests_reach():
    """What test_gpu_batch_ahead.py, test_gpu_bbb_run.py and the 784-200-10 baseline reach of this table, from their shapes:
    S = 4 (and 16 at the bench shape) only, no S = 1, 2 or 8, no batch of one row, no run that cannot assemble ahead, no
    misaligned buffer, no prior vector, no slot0 in a first call, none of the SWAG cells."""
    old = {name: rc.reached_cells(c) for name, c in rc.old_run_shapes().items()}
    for name, c in rc.old_run_shapes().items():
        print(f"OLD | {name} | S={c.S} fwd tiles {rc.fwd_tile_grid(c.dims, c.bmax)} | " + "; ".join(sorted(old[name])))
    reached = set().union(*old.values())
    at = sorted({int(c.split("S=")[1].split()[0]) for c in reached if " chained S=" in c})
    assert at == [4] or at == [4, 16], at
    assert not any(c.startswith("SWAG") for c in reached - {"SWAG frequency 1", "SWAG frequency >1"})
    for cell in ("no batch-ahead: one layer", "no batch-ahead: unfused", "state buffers 4 bytes off 16-byte alignment",
                 "BBB prior vectors", "slot0 > 0", "fwd_tiles == 8", "XCD residue without tiles", "prep XCD branch fwd_tiles&7!=0"):
        assert cell not in reached, cell
    assert not any(c.endswith("batch 1") for c in reached)
    assert len(CELLS - reached) >= 40


# ---------------------------------------------------------------- the run reference against the oracle modules
@pytest.mark.parametrize("name", ["r_s2", "r_s8_xcd8_l3_mse", "r_s4_scalar_copy"])
def test_run_reference_equals_the_oracle_modules(name):
    """A whole short run in float64, state handed on unrounded: bit for bit oracle.sgd / swag / sgld / bbb."""
    case = rc.CASE_BY_NAME[name]
    data, spec, d = data_of(case), case.spec, data_of(case).step
    same = lambda u, v: np.array_equal(np.asarray(u), np.asarray(v)) and np.asarray(u).dtype == np.float64
    batch = lambda call, i: data.tab[call.slot0 + i, :call.sizes[i]]
    for mode in MODES:
        call = case.call(mode, val=(mode == "bbb"))
        s = rc.initial_state(mode, data, call.k)
        if mode == "sgd":
            st = o_sgd.SGDState(s["theta"])
        elif mode == "sgld":
            st = o_sgld.SGLDState(s["theta"])
            st.mean, st.sq_mean, st.n = s["mean"].astype(np.float64), s["sq"].astype(np.float64), call.n0
        elif mode == "swag":
            st = o_swag.SWAGState(s["theta"], call.k)
            st.mean, st.sq_mean, st.n = s["mean"].astype(np.float64), s["sq"].astype(np.float64), call.n0
            st.dev = s["dev"][:min(cdiv(call.n0, call.freq), call.k)].astype(np.float64)
        else:
            mu, rho = s["mu"].astype(np.float64), s["rho"].astype(np.float64)
        for i in range(rc.N_STEPS):
            rows = batch(call, i)
            x, y = d.x[rows], d.y[rows]
            out = ref_run_step(case, data, call, mode, i, s)
            assert out["slot"] == call.slot0 + i
            if mode == "sgd":
                loss, _ = o_sgd.sgd_step(st, x, y, spec, call.lrs[i])
                assert same(out["theta"], st.theta) and same(out["loss"], loss)
            elif mode == "sgld":
                loss, _ = o_sgld.sgld_step(st, x, y, spec, call.lrs[i], o_philox.normal(case.seed, sc.STREAM["sgld"], call.n0 + i, case.D))
                assert same(out["theta"], st.theta) and same(out["mean"], st.mean) and same(out["sq"], st.sq_mean) and same(out["loss"], loss)
            elif mode == "swag":
                loss = o_swag.swag_step(st, x, y, spec, call.lrs[i], frequency=call.freq)
                assert same(out["theta"], st.theta) and same(out["mean"], st.mean) and same(out["sq"], st.sq_mean) and same(out["loss"], loss)
                assert same(out["dev"][:st.dev.shape[0]], st.dev) and same(out["dev"][st.dev.shape[0]:], s["dev"][st.dev.shape[0]:].astype(np.float64))
            else:
                pm, pr = (d.pm_vec, d.pr_vec) if case.prior_vec else case.step.prior
                eps = o_philox.normal(case.seed, sc.STREAM["bbb"], call.n0 + i, case.D)
                ref = o_bbb.bbb_step(mu, rho, eps, x, y, spec, call.lrs[i], case.step.alpha, pm, pr)
                mu, rho = ref["mu"], ref["rho"]
                assert same(out["mu"], mu) and same(out["rho"], rho) and same(out["w"], ref["w"])
                assert same(out["cost"], np.array([ref["cost"], ref["loss"], ref["kl"]]))
                if (call.n0 + i) % 10:
                    assert same(out["val"], o_bbb.validation_loss(ref["w"], data.xv, data.yv, spec))
                else:
                    assert out["val"] is None
            s = rc.next_state(s, out)
        if mode == "swag":
            assert st.n == call.n0 + rc.N_STEPS and st.dev.shape[0] == min(cdiv(st.n, call.freq), call.k)


# ---------------------------------------------------------------- float32 reference passes, wrong references fail
def calls_of(case, mode):
    """The calls the CPU comparison covers: the short ragged run (BBB: with validation) and the bookkeeping runs of the case."""
    out = [("ragged", case.call(mode, val=(mode == "bbb")), rc.initial_state)]
    for b in BOOKS:
        if b.case == case.name and b.mode == mode:
            out.append((b.name, rc.book_call(b)[1][-1], rc.initial_state))
    return out


PAIRS = [(c, m) for c in CASES for m in c.modes]


@pytest.mark.parametrize("case,mode", PAIRS, ids=[f"{c.name}-{m}" for c, m in PAIRS])
def test_comparison_passes_the_float32_reference_and_fails_every_wrong_reference(case, mode):
    data = data_of(case)
    for label, call, init in calls_of(case, mode):
        s0 = init(mode, data, call.k)
        states, worst = [], {}
        for i in range(len(call.sizes)):      # as on the device: the reference restarts from the stored state of every step
            ref = ref_run_step(case, data, call, mode, i, s0)
            got = rc.stored(ref_run_step(case, data, call, mode, i, s0, np.float32))
            rep = compare_run_step(case, data, call, mode, i, s0, got, ref, what=f"float32 reference, {label}: ")
            for q, r in rep.items():
                worst[q] = max(worst.get(q, 0.0), r)
            states.append(s0)
            s0 = rc.next_state(s0, got)
        for q, r in sorted(worst.items()):     # (profiles/run_matrix/float32_oracle_tolerances.txt: run with -s)
            print(f"FLOAT32 | {case.name} | {mode} | {label} | {q} | error / tolerance {r:.4f}")
            assert r <= 1.0
        for mutation in RUN_MUTATIONS:
            if not rc.run_mutation_applies(case, call, mode, mutation):
                continue
            caught = None
            for i, s in enumerate(states):
                ref = ref_run_step(case, data, call, mode, i, s)
                got = rc.stored(ref_run_step(case, data, call, mode, i, s, np.float32, mutation=mutation))
                try:
                    compare_run_step(case, data, call, mode, i, s, got, ref)
                except AssertionError as e:
                    caught = (i, str(e).splitlines()[0][:200])
                    break
            assert caught, f"{case.name} {mode} {label}: the comparison does not see the wrong reference '{mutation}'"
            print(f"WRONG | {case.name} | {mode} | {label} | {mutation} | step {caught[0]} | {caught[1]}")


def test_every_wrong_reference_is_exercised_and_the_floor_row_is_the_ceil_row():
    for mutation, modes in RUN_MUTATIONS.items():
        n = sum(rc.run_mutation_applies(c, call, m, mutation) for c in CASES for m in modes if m in c.modes
                for _, call, _ in calls_of(c, m))
        if mutation in rc.EQUIVALENT_MUTATIONS:
            assert n == 0
            continue
        assert n >= (2 if mutation in ("BBB prior vector ignored", "SWAG hit tested on n+1") else len(rc.FUSED_CASES)), (mutation, n)
    assert len(RUN_MUTATIONS) == 10
    # a hit has n % frequency == 0, where floor and ceil of n / frequency agree: the same reference, bit for bit
    for f in range(1, 8):
        for n in range(0, 60):
            if n % f == 0:
                assert n // f == cdiv(n, f)
    case = rc.CASE_BY_NAME["r_s2"]
    data, call = data_of(case), case.call("swag")
    s = rc.initial_state("swag", data, call.k)
    for i in range(rc.N_STEPS):
        a = ref_run_step(case, data, call, "swag", i, s)
        b = ref_run_step(case, data, call, "swag", i, s, mutation="SWAG row by floor instead of ceil")
        assert all(np.array_equal(a[k], b[k]) for k in s)
        s = rc.next_state(s, a)
