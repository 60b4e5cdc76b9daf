"""The HMC case table (tests/hmc_cases.py) against the library's source, on the CPU.

The constants and expressions of `pyz_hmc_step`'s choice are read out of pyz_api.hip, pyz_hmc_fused.h and pyz_hmc_multi.h
and compared with the plain-Python restatement; the boundaries are pinned as literal values; the cells the cases reach
are compared with the coverage table cell by cell, so deleting a case or moving a threshold fails here with the name of
the lost cell; the data of every case is checked to be what the GPU matrix relies on; and, per case, the comparison the
GPU matrix uses is shown to pass the float32 oracle and to fail each of eight deliberately wrong oracles."""

import os
import re

import numpy as np
import pytest

import hmc_cases as hc
from hmc_cases import CASES, CELLS, case_data, check_chains, compare, dispatch, expected_path, reached_cells

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesian_inference_for_nn_amd", "csrc")

# cases for which a wrong oracle cannot be made to fail the comparison: {case name: {mutation: reason}} (at most one case in ten)
SENSITIVITY_EXEMPT = {}


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


def hmc_step_body():
    api = src("pyz_api.hip")
    i = api.index("int pyz_hmc_step(")
    return api[i:api.index("\n}", i)]


# ---------------------------------------------------------------- the restatement against the source
def test_constants_and_environment_defaults_match_the_source():
    fused, multi, body = src("pyz_hmc_fused.h"), src("pyz_hmc_multi.h"), hmc_step_body()
    assert "#define PYZ_HF_MAXI %d\n" % hc.HF_MAXI in fused and "#define PYZ_HF_MAXC %d\n" % hc.HF_MAXC in fused
    assert "#define PYZ_HF_WAVES %d\n" % hc.HF_WAVES in fused and "#define PYZ_HF_THREADS %d\n" % (64 * hc.HF_WAVES) in fused
    assert "#define PYZ_HM_WAVES %d\n" % hc.HM_WAVES in multi and "#define PYZ_HM_MAXW %d\n" % hc.HM_MAXW in multi
    assert "#define PYZ_STREAM_HMC %du" % hc.STREAM_HMC in src("pyz_rng.h")
    defaults = {"PYZ_HMC_FUSED": 1, "PYZ_HMC_MULTI": 1, "PYZ_HMC_ROWS_PER_WG": hc.ROWS_PER_WG,
                "PYZ_HMC_MULTI_MAX_CHAINS": hc.MULTI_MAX_CHAINS, "PYZ_HMC_RESIDENT": 1, "PYZ_HMC_GRAPH": 1}
    for name, value in defaults.items():
        assert env_default(body, name) == value, name
        # read per call, not once per process: the cases (and the library's other tests) flip them between calls
        assert not re.search(r'static[^;]*pyz_env_int\("%s"' % name, body), name
    assert 'pyz_env_int("PYZ_HMC_SPIN_LIMIT", 1 << 20)' in body
    assert set(defaults) | {"PYZ_HMC_SPIN_LIMIT"} == set(hc.PER_CALL_ENV) | set(hc.ENV_FORBIDDEN)
    assert body.count("150 * 1024") == 2 and hc.LDS_LIMIT == 150 * 1024      # multi_ok and the eligibility condition
    assert body.count("64 * 1024") == 3 and hc.LDS_ATTR == 64 * 1024         # kmulti, kres, kern


def test_lds_formulas_match_the_source():
    fused, multi = squash(src("pyz_hmc_fused.h")), squash(src("pyz_hmc_multi.h"))
    assert ("return(size_t)(4+PYZ_HF_WAVES)*D+(size_t)64*(MI+MC+2)+(size_t)N*MI+(size_t)N*MC+"
            "(size_t)N*(loss==PYZ_LOSS_MSE?C:1);") in fused
    assert "return((pyz_hmc_fused_floats(N,MI,MC,C,D,loss)*4+15)/16)*16+64*sizeof(double);" in fused
    assert ("constsize_tfl=(size_t)(3+PYZ_HM_WAVES)*D+(size_t)64*(MI+MC+2)+(size_t)max_rows*MI+(size_t)max_rows*MC+"
            "(size_t)max_rows*(loss==PYZ_LOSS_MSE?C:1);return((fl*4+15)/16)*16+64*sizeof(double);") in multi
    # the moons model of HMC_classification.py and one slice of it
    assert hc.fused_lds_bytes(1600, 2, 2, 2, 252, False) == 54208 and hc.multi_lds_bytes(101, 2, 2, 2, 252, False) == 11136
    assert hc.multi_lds_bytes(356, 8, 8, 8, 960, True) == 66176


def test_dispatch_expressions_match_the_source():
    body = squash(hmc_step_body())
    assert "constintI=m->dims[0],H=m->dims[1],C=m->L==2?m->dims[2]:0;" in body
    assert "constintMIC=(I<=2&&C<=2)?2:((I<=4&&C<=4)?4:8);" in body
    assert "constintbucket=(I<=2&&C<=2)?0:((I<=4&&C<=4)?1:2);" in body
    assert "constsize_tlds=m->L==2?pyz_hmc_fused_lds_bytes(n_rows,MIC,MIC,C,(int)m->D,m->loss):0;" in body
    assert 'constintrows_per_wg=std::max(16,pyz_env_int("PYZ_HMC_ROWS_PER_WG",96));' in body
    assert "constintNW=std::min(PYZ_HM_MAXW,n_rows/rows_per_wg);" in body
    assert "constsize_tmlds=m->L==2?pyz_hmc_multi_lds_bytes(cdiv(n_rows,std::max(NW,1))+1,MIC,MIC,C,(int)m->D,m->loss):0;" in body
    assert 'constboolmulti_ok=allow_multi&&NW>=2&&P<=pyz_env_int("PYZ_HMC_MULTI_MAX_CHAINS",16)&&mlds<=150*1024;' in body
    assert ("if(allow_fused&&!d_prior_mean_vec&&!d_prior_sigma_vec&&m->L==2&&I<=PYZ_HF_MAXI&&C<=PYZ_HF_MAXC&&H+C<=64&&"
            "(lds<=150*1024||multi_ok)&&m->acts[0]!=PYZ_ACT_SOFTMAX){") in body
    assert "mm.max_rows=cdiv(n_rows,NW)+1;" in body
    assert 'boolresident=pyz_env_int("PYZ_HMC_RESIDENT",1)!=0&&NW*P<=pyz_cu_count();' in body
    assert "if(!use_graph||st==nullptr){" in body
    assert "if(multi_ok){" in body and body.index("if(multi_ok){") < body.index("PYZ_LAUNCH(kern,dim3(P),dim3(PYZ_HF_THREADS),lds,st,f);")
    for k in ("kmulti", "kres"):
        assert f"if(mlds>64*1024)PYZ_HIP(hipFuncSetAttribute(reinterpret_cast<constvoid*>({k})," in body
    assert "if(lds>64*1024)PYZ_HIP(hipFuncSetAttribute(reinterpret_cast<constvoid*>(kern)," in body
    # the slices of the kernels themselves
    multi = squash(src("pyz_hmc_multi.h"))
    assert multi.count("constintr0=(int)(((longlong)N*wg)/NW),r1=(int)(((longlong)N*(wg+1))/NW),nloc=r1-r0;") == 2


def test_pick_macros_and_their_arms_match_the_source():
    body = hmc_step_body()
    sq = squash(body)
    for macro, var, kernel in (("PYZ_HF_PICK", "kern", "k_hmc_fused"), ("PYZ_HM_PICK", "kmulti", "k_hmc_multi"),
                               ("PYZ_HR_PICK", "kres", "k_hmc_resident")):
        assert (f"#define{macro}(ACT)\\{var}=bucket==0?{kernel}<2,2,ACT>:(bucket==1?{kernel}<4,4,ACT>:{kernel}<8,8,ACT>)") in sq, macro
        arms = re.findall(r"case (PYZ_ACT_\w+): %s\((PYZ_ACT_\w+)\); break;" % macro, body)
        assert arms == [("PYZ_ACT_RELU",) * 2, ("PYZ_ACT_TANH",) * 2, ("PYZ_ACT_SIGMOID",) * 2], (macro, arms)
        assert f"default: {macro}(PYZ_ACT_LINEAR); break;" in body, macro
        assert f"#undef {macro}" in body
    assert hc.ACT_ARMS == ("relu", "tanh", "sigmoid", "linear")


def test_launch_sequences_match_the_source():
    body = hmc_step_body()
    sq = squash(body)
    assert "if(resident){PYZ_LAUNCH(kres,dim3(NW,P),dim3(PYZ_HM_THREADS),mlds,st,mm);return;}" in sq
    assert ("for(intt=0;t<=L;++t){mm.t=t;PYZ_LAUNCH(kmulti,dim3(NW,P),dim3(PYZ_HM_THREADS),mlds,st,mm);}"
            "PYZ_LAUNCH(k_hmc_multi_final,dim3(P),dim3(PYZ_HM_THREADS),0,st,mm);") in sq
    generic = body[body.index("if ((rc = set_ctl("):]
    sites = re.findall(r"PYZ_LAUNCH\((\w+),", generic)
    assert sites == ["k_loss_finalize", "k_hmc_begin", "k_hmc_energy_finalize", "k_hmc_kick_drift", "k_hmc_kick_drift",
                     "k_hmc_kick_drift", "k_hmc_end_energy", "k_hmc_energy_finalize", "k_hmc_accept", "k_hmc_restore"], sites
    assert set(re.findall(r"PYZ_LAUNCH\((\w+),", body)) == set(hc.HMC_SITES)
    for L in (0, 1, 3):
        seq = dispatch((4, 10, 6, 3), ("tanh", "relu", "softmax"), "scce", 100, 2, L).launches
        assert seq.count("k_hmc_kick_drift") == L + 1 and seq.count("k_loss_finalize") == L + 1 and len(seq) == 2 * L + 8
        assert dispatch((2, 50, 2), ("relu", "softmax"), "scce", 1600, 1, L, env=hc.NO_RES).launches == ("kmulti",) * (L + 1) + ("k_hmc_multi_final",)
    assert dispatch((2, 50, 2), ("relu", "softmax"), "scce", 1600, 1, 20).launches == ("kres",)
    assert dispatch((2, 50, 2), ("relu", "softmax"), "scce", 100, 1, 20).launches == ("kern",)


def test_philox_streams_match_the_source():
    for name in ("pyz_kernels.h", "pyz_hmc_fused.h", "pyz_hmc_multi.h"):
        assert "PYZ_STREAM_HMC + 16u * (uint32_t)" in src(name), name


# ---------------------------------------------------------------- literal boundaries
MOONS = ((2, 50, 2), ("relu", "softmax"), "scce")
WIDE = ((8, 56, 8), ("relu", "softmax"), "scce")


def path_of(model, rows, P=1, L=1, **kw):
    return dispatch(*model, rows, P, L, **kw)


def test_slice_count_boundaries_are_pinned():
    first = lambda nw: next(n for n in range(1, 10000) if path_of(MOONS, n).NW == nw)
    assert [first(nw) for nw in (2, 17, 32)] == [192, 1632, 3072]
    assert path_of(MOONS, 191).path == "fused" and path_of(MOONS, 191).NW == 0 and path_of(MOONS, 192).path == "resident"
    assert path_of(MOONS, 8192).NW == 32 and sum(path_of(MOONS, 8191).slices) == 8191
    assert path_of(MOONS, 289).slices == (96, 96, 97) and path_of(MOONS, 479).slices == (119, 120, 120, 120)
    assert set(path_of(MOONS, 1640).slices) == {96, 97} and len(path_of(MOONS, 1640).slices) == 17


def test_lds_boundaries_are_pinned():
    largest = lambda model: max(n for n in range(1, 20000) if path_of(model, n, env=hc.NO_MULTI).path == "fused")
    assert largest(MOONS) == 6569 and largest(WIDE) == 1054
    assert path_of(WIDE, 1055, env=hc.NO_MULTI).path == "generic" and path_of(WIDE, 1055).path == "resident"
    assert path_of(MOONS, 6570).path == "resident"     # too large for one workgroup, sliced all the same
    wide_mse = ((8, 56, 8), ("linear", "linear"), "mse")
    first_attr = next(n for n in range(3072, 20000) if path_of(wide_mse, n).mlds > hc.LDS_ATTR)
    assert first_attr == 11137 and path_of(wide_mse, 11136).mlds <= hc.LDS_ATTR
    assert path_of(wide_mse, 8192).mlds < hc.LDS_ATTR   # why one case has more than 8192 rows


def test_shape_limits_are_pinned():
    m = lambda dims: (dims, ("tanh", "softmax"), "scce")
    assert path_of(m((8, 56, 8)), 100).path == "fused" and path_of(m((4, 57, 8)), 100).path == "generic"
    assert path_of(m((8, 20, 4)), 100).path == "fused" and path_of(m((9, 20, 4)), 100).path == "generic"
    assert path_of(m((3, 12, 8)), 100).path == "fused" and path_of(m((3, 12, 9)), 100).path == "generic"
    assert path_of(MOONS, 100, vec_prior=True).path == "generic" and path_of(MOONS, 100, env=hc.NO_FUSED).path == "generic"
    assert path_of(((4, 10, 6, 3), ("tanh", "relu", "softmax"), "scce"), 1000).path == "generic"
    assert [hc.bucket(I, C) for I, C in ((1, 1), (2, 2), (3, 2), (2, 3), (4, 4), (5, 1), (1, 5), (8, 8))] == [0, 0, 1, 1, 1, 2, 2, 2]


def test_chain_count_boundaries_are_pinned():
    assert path_of(MOONS, 1600, P=16).path == "resident" and path_of(MOONS, 1600, P=17).path == "fused"
    assert path_of(MOONS, 1600, P=16).NW == 16                                    # 16 x 16 = 256
    assert path_of(MOONS, 1640, P=16).NW == 17 and path_of(MOONS, 1640, P=16).path == "multi"   # 272 > 256
    assert path_of(MOONS, 1640, P=15).path == "resident"                          # 255
    assert path_of(MOONS, 1600, P=4, cu_count=64).path == "resident" and path_of(MOONS, 1600, P=5, cu_count=64).path == "multi"
    assert path_of(MOONS, 1600, P=4, env=hc.NO_RES).path == "multi" and path_of(MOONS, 1600, P=4, env=hc.NO_MULTI).path == "fused"
    assert path_of(MOONS, 1600).graph and not path_of(MOONS, 1600, env={"PYZ_HMC_GRAPH": "0"}).graph and not path_of(MOONS, 100).graph


# ---------------------------------------------------------------- the cases against the table
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_cell_is_reached(cell):
    assert any(cell in reached_cells(c) for c in CASES), f"no case reaches the cell '{cell}'"


def test_no_case_went_missing_and_the_table_has_its_cells():
    """Several cells are reached by more than one case: removing one of those loses no cell, so the count is pinned."""
    assert len(CASES) == 52 and len({c.name for c in CASES}) == 52
    assert len(CELLS) == 120
    assert sum(bool(re.match(r"(fused|multi|resident) <\d,\d> ", c)) for c in CELLS) == 36
    assert sum(" head " in c for c in CELLS) == 12 and sum(" L=" in c for c in CELLS) == 16
    assert sum(" momentum " in c for c in CELLS) == 8 and sum(c.endswith("prior mean!=0 sigma!=1") for c in CELLS) == 4


def test_every_case_is_small_and_uses_only_the_documented_switches():
    for c in CASES:
        assert c.rows <= 8192 or c.name == hc.BIG_LDS_CASE, c.name
        assert c.P <= 80 and c.L <= 20 and c.rows <= 11360, c.name
        assert set(c.env) <= set(hc.PER_CALL_ENV), c.name
        assert all(v == "0" for v in c.env.values()), c.name
        assert float(np.float32(c.eps)) == c.eps, c.name        # the library's float is the oracle's number
        assert not c.vec_prior or expected_path(c).path == "generic"
    big = hc.CASE_BY_NAME[hc.BIG_LDS_CASE]
    assert expected_path(big).mlds > hc.LDS_ATTR and expected_path(big._replace(rows=8192)).mlds < hc.LDS_ATTR


def test_expected_path_of_known_cases():
    p = expected_path(hc.CASE_BY_NAME["res_b0_relu_c3"])
    assert (p.path, p.bucket, p.NW, p.launches, p.graph) == ("resident", 0, 16, ("kres",), True) and set(p.slices) == {100}
    p = expected_path(hc.CASE_BY_NAME["multi_b0_relu_over_cu"])
    assert (p.path, p.NW, len(p.launches)) == ("multi", 17, 5)
    assert expected_path(hc.CASE_BY_NAME["multi_b0_relu_over_cu"], cu_count=304).path == "resident"
    assert expected_path(hc.CASE_BY_NAME["fused_b0_sigmoid_17_chains"]).path == "fused"
    assert expected_path(hc.CASE_BY_NAME["fused_b0_sigmoid_17_chains"], P=1).path == "resident"
    assert expected_path(hc.CASE_BY_NAME["gen_lds_over"]).path == "generic"
    assert expected_path(hc.CASE_BY_NAME["fused_b2_relu_lds_under"]).lds == 153600 == hc.LDS_LIMIT   # exactly at the limit: the condition is <=


# ---------------------------------------------------------------- the data, the tolerances and the sensitivity of the comparison
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_data_properties(case):
    a, b = case_data(case), case_data(case)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert a.q0.shape == (case.P, case.D) and a.q0.dtype == np.float32 and a.z.shape == (case.P, case.D) and a.z.dtype == np.float32
    assert a.x.shape == (case.rows, case.dims[0]) and a.x.dtype == np.float32 and np.all(np.isfinite(a.q0)) and np.all(np.isfinite(a.z))
    if case.loss == "scce":
        assert a.y.dtype == np.int32 and a.y.min() >= 0 and a.y.max() < case.dims[-1]
    within, dead = hc.hidden_stats(case, a)
    for l, act in enumerate(case.acts[:-1]):
        if act in ("tanh", "sigmoid"):
            assert within[l] >= 0.9, f"{case.name}: layer {l} ({act}): only {within[l]:.2f} of the pre-activations within +-4"
        if act == "relu":
            assert dead[l] <= 0.5, f"{case.name}: layer {l}: {dead[l]:.2f} of the relu units dead over the data set"
    us = hc.uniforms(case, a)
    refs = [hc.oracle_result(case, a, c) for c in check_chains(case.P)]
    if case.prior[1] < 0:
        assert all(np.isnan(r["log_ratio"]) and not r["accepted"] for r in refs)
    else:
        assert all(abs(r["log_ratio"]) < 5.0 for r in refs), [r["log_ratio"] for r in refs]
        flags = [r["accepted"] for r in refs]
        assert flags == [(c % 2 == 0) != (case.reject0 and c == 0) for c in check_chains(case.P)]
        if case.P >= 2:
            assert any(flags) and not all(flags), f"{case.name}: accepted and rejected chains must both occur"
        for r, c in zip(refs, check_chains(case.P)):      # a factor of two on either side of the decision
            ratio = np.exp(r["log_ratio"])
            assert us[c] <= 0.5 * ratio * 1.001 or us[c] >= 2.0 * ratio


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_comparison_passes_the_float32_oracle_and_fails_every_wrong_oracle(case):
    data = case_data(case)
    chains = check_chains(case.P)
    refs = {c: hc.oracle_result(case, data, c) for c in chains}
    rel32 = hc.tolerances(case)
    rows = []
    for c in chains:
        report = compare(hc.oracle_result(case, data, c, np.float32), refs[c], case, what=f"float32 oracle, chain {c}: ")
        for k, (err, tol) in report.items():
            rows.append((k, err, tol))
    for k in sorted(rel32):      # (the table of the pull request: run with -s)
        tols = [t for kk, _, t in rows if kk == k]
        print(f"TOLERANCE | {case.name} | {expected_path(case).path} | {k} | float32 oracle {rel32[k]:.2e} of the scale | "
              f"tolerance {min(tols) if tols else float('nan'):.3e} .. {max(tols) if tols else float('nan'):.3e}")
    for k, (_, _, scale, floor) in hc.quantities(refs[chains[0]], refs[chains[0]], case).items():
        if np.isfinite(scale):     # a tolerance below the rounding of what is stored could not be met by any kernel
            assert floor <= hc.CAP * scale, f"{case.name}: {k}: the float32 rounding {floor:.2e} exceeds 1e-4 of the scale {scale:.2e}"
    exempt = SENSITIVITY_EXEMPT.get(case.name, {})
    for mutation in hc.MUTATIONS:
        applies = [c for c in chains if hc.mutation_applies(case, mutation, c)]
        if not applies or mutation in exempt:
            continue
        caught = []
        for c in applies:
            try:
                compare(hc.oracle_result(case, data, c, np.float64, mutation=mutation), refs[c], case)
            except AssertionError as e:
                caught.append(str(e))
                break
        assert caught, f"{case.name}: the comparison does not see the wrong oracle '{mutation}'"


def test_every_wrong_oracle_is_exercised_and_few_cases_are_exempt():
    assert len(SENSITIVITY_EXEMPT) * 10 <= len(CASES) and set(SENSITIVITY_EXEMPT) <= set(hc.CASE_BY_NAME)
    for mutation in hc.MUTATIONS:
        n = sum(any(hc.mutation_applies(c, mutation, ch) for ch in check_chains(c.P)) and mutation not in SENSITIVITY_EXEMPT.get(c.name, {})
                for c in CASES)
        assert n >= 8, (mutation, n)
    sliced = [c for c in CASES if expected_path(c).NW]
    assert all(hc.mutation_applies(c, "drop_last_row_of_first_slice", 0) for c in sliced) and len(sliced) == 28
