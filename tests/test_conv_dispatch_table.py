"""The conv case table (tests/conv_checks.py) against the library's source, on the CPU.

The rules that decide how k_conv_fwd, k_conv_wgrad, k_conv_wgrad_reduce and k_conv_dgrad are launched (conv_waves,
stem_rows_per_range, the range count, the chunk walk, the tile counts, what stem_backward hands the data gradient) are
read out of pyz_api.hip / pyz_conv.h and compared with the plain-Python restatement of conv_checks; the cells the cases
and the dedicated shapes of tests/test_gpu_conv_paths.py reach are compared with LAUNCH_CELLS, and every new case and
every dedicated shape must be the only one that reaches some cell: deleting a case or moving a threshold fails here
with the name of the lost cell.  The probe reports kernel names only, not block sizes, so this is what ties a case to
its path."""

import os
import re

import pytest

import conv_checks as cc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesian_inference_for_nn_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def function_body(text, head):
    i = text.index(head)
    return text[i:text.index("\n}", i)]


def code_lines(body):
    return [l.strip() for l in body.splitlines() if l.strip() and not l.strip().startswith("//")]


CONV, API = src("pyz_conv.h"), src("pyz_api.hip")
EVERYTHING = cc.ALL + tuple(cc.PATH_SHAPES)


def launches_of(name):
    if name in cc.PATH_SHAPES:
        case, max_batch = cc.path_case(name)
        return {b: cc.conv_launches(case.shape, case.ops, b, max_batch) for b in case.batches}
    case = cc.CASES[name]
    return {b: cc.conv_launches(case.shape, case.ops, b, b + cc.PLAN_SLACK) for b in case.batches}


# ---------------------------------------------------------------- the restatement against the source
def test_constants_match_the_header():
    for name, value in (("PYZ_CONV_MAX_K", cc.CONV_MAX_K), ("PYZ_CONV_WAVES", cc.CONV_WAVES), ("PYZ_WGRAD_CHUNK", cc.WGRAD_CHUNK)):
        assert re.findall(r"#define %s (\d+)\b" % name, CONV) == [str(value)], name
    assert re.findall(r"#define PYZ_CONV_MAX_ROWS \(1 << (\d+)\)", CONV) == ["24"] and cc.CONV_MAX_ROWS == 1 << 24
    from bayesian_inference_for_nn_amd import engine
    assert engine.CONV_MAX_K == cc.CONV_MAX_K


def test_wave_and_range_rules_match_the_source_line_by_line():
    assert code_lines(function_body(API, "inline int conv_waves("))[1:] == [
        "int S = 1;",
        "while (S < PYZ_CONV_WAVES && tiles * S < 1024 && steps >= 16 * S) S *= 2;",
        "return S;"]
    assert code_lines(function_body(API, "inline int stem_rows_per_range("))[1:] == [
        "const long long m_max = (long long)s->max_batch * o.OH * o.OW;",
        "return (int)std::max<long long>(256, ((m_max + 255) / 256 + 1) / 2 * 2);"]
    fwd = function_body(API, "void stem_forward(")
    for text in ("const long long tiles = (long long)((g.M + 31) / 32) * ((g.N + 31) / 32);",
                 "const int S = conv_waves(tiles * P, g.KT / 2);",
                 "PYZ_LAUNCH(k_conv_fwd, dim3((unsigned)tiles, P), dim3(64 * S), (size_t)g.KT * 8 + (S > 1 ? S * 4096 : 0), st, g);"):
        assert text in fwd, text
    bwd = function_body(API, "void stem_backward(")
    for text in ("g.rows_per_g = stem_rows_per_range(s, c);",
                 "g.G = cdiv(g.M, g.rows_per_g);",
                 "const long long tiles = (long long)((g.K + 1 + 31) / 32) * ((g.N + 31) / 32);",
                 "const int S = conv_waves(tiles * g.G * P, std::min(g.M, g.rows_per_g) / 2);",
                 "PYZ_LAUNCH(k_conv_wgrad, dim3((unsigned)(tiles * g.G), P), dim3(64 * S), (S > 1 ? S * 4096 : 0) + PYZ_WGRAD_CHUNK * 16, st, g);",
                 "PYZ_LAUNCH(k_conv_wgrad_reduce, dim3((unsigned)cdiv((long long)(g.K + 1) * g.N, 16), P), dim3(256), 0, st, g);",
                 "if (o > 0) {",
                 "g.below = b.kind == PYZ_STEM_CONV ? b.out : nullptr;",
                 "g.below_pstride = g.out_pstride;",
                 "g.act_below = b.act;",
                 "PYZ_LAUNCH(k_conv_dgrad, dim3((unsigned)cdiv((long long)batch * c.H * c.W * c.C, 256), P), dim3(256), 0, st, g);"):
        assert text in bwd, text
    args = function_body(API, "ConvArgs conv_args(")
    assert "g.M = batch * c.OH * c.OW;" in args
    # what pyz_stem_create derives per conv: the pads, the output map, K and KT, and the two limits
    create = function_body(API, "int pyz_stem_create(")
    for text in ("const int ph = d[4] ? c.kh - 1 : 0, pw = d[4] ? c.kw - 1 : 0;", "c.pt = ph / 2;", "c.pl = pw / 2;",
                 "if (c.kh > H + ph || c.kw > W + pw)", "c.OH = H + ph - c.kh + 1;", "c.OW = W + pw - c.kw + 1;",
                 "if ((long long)c.kh * c.kw * C > PYZ_CONV_MAX_K)", "c.K = c.kh * c.kw * C;", "c.KT = (c.K + 2) & ~1;",
                 "if ((long long)max_batch * c.OH * c.OW > PYZ_CONV_MAX_ROWS || (long long)max_batch * H * W * C >= (1LL << 31) ||"):
        assert text in create, text


def test_kernel_arithmetic_matches_the_source():
    fwd = function_body(CONV, "k_conv_fwd(ConvArgs g)")
    for text in ("float *red = lds + 2 * g.KT;", "const int tiles_n = (g.N + 31) >> 5;",
                 "const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n, p = blockIdx.y;",
                 "const int steps = g.KT >> 1;", "0, (steps - w + S - 1) / S, acc,", "const int k = 2 * (w + S * u) + h;"):
        assert text in fwd, text
    wg = function_body(CONV, "k_conv_wgrad(ConvArgs g)")
    for text in ("const int tiles_n = (g.N + 31) >> 5, tiles = ((g.K + 1 + 31) >> 5) * tiles_n;",
                 "const int rg = blockIdx.x / tiles, tile = blockIdx.x - rg * tiles, p = blockIdx.y;",
                 "const int tk = tile / tiles_n, tn = tile - tk * tiles_n;",
                 "const int m0 = rg * g.rows_per_g, m1 = min(M, m0 + g.rows_per_g);",
                 "for (int c0 = m0; c0 < m1; c0 += PYZ_WGRAD_CHUNK) {",
                 "const int rows = min(PYZ_WGRAD_CHUNK, m1 - c0);",
                 "if (c0 > m0) __syncthreads();",
                 "const int steps = (rows + 1) >> 1;", "0, (steps - w + S - 1) / S, acc,", "const int e = 2 * (w + S * u) + h;",
                 "if (e < rows) {",
                 "float *op = g.part + (((long long)p * g.G + rg) * tiles + tile) * 1024;"):
        assert text in wg, text
    red = function_body(CONV, "k_conv_wgrad_reduce(ConvArgs g)")
    for text in ("const int N = g.N, E = (g.K + 1) * N;", "const int e = blockIdx.x * 16 + el;",
                 "const int tiles_n = (N + 31) >> 5, tiles = ((g.K + 1 + 31) >> 5) * tiles_n;",
                 "const int tile = (k >> 5) * tiles_n + (n >> 5), idx = (k & 31) * 32 + (n & 31);",
                 "for (int rg = q; rg < g.G; rg += 16) s += pp[(long long)rg * tiles * 1024];"):
        assert text in red, text
    dg = function_body(CONV, "k_conv_dgrad(ConvArgs g)")
    for text in ("const int oy = y - i + g.pt;", "if ((unsigned)oy >= (unsigned)g.OH) continue;", "const int ox = x - j + g.pl;",
                 "if ((unsigned)ox >= (unsigned)g.OW) continue;",
                 "if (g.below) s *= pyz_act_grad(g.below[p * g.below_pstride + e], g.act_below);"):
        assert text in dg, text


def test_rules_at_their_edges():
    assert [cc.conv_waves(1, s) for s in (15, 16, 31, 32, 64, 4096)] == [1, 2, 2, 4, 4, 4]
    assert [cc.conv_waves(t, 100) for t in (255, 256, 511, 512, 1023, 1024)] == [4, 4, 4, 2, 2, 1]
    # forward S = 4 needs KT / 2 >= 32 steps: K >= 62 (D's 72 takes it while its tiles stay under 256)
    assert [cc.conv_waves(2, ((K + 2) & ~1) // 2) for K in (27, 29, 30, 61, 62, 144, 4094)] == [1, 1, 2, 2, 4, 4, 4]
    # a range outgrows one chunk of 512 rows only when max_batch * OH * OW > 131 072: 129 images of 32 x 32
    assert [cc.rows_per_range(mb, 32, 32) for mb in (1, 36, 64, 65, 127, 128, 129, 130)] == [256, 256, 256, 260, 508, 512, 516, 520]
    assert cc.rows_per_range(200, 31, 31) == 752 and cc.rows_per_range(4097, 63, 65) == 65536
    assert cc.wave_steps(73, 4) == [19, 18, 18, 18] and cc.wave_steps(1, 4) == [1, 0, 0, 0] and cc.wave_steps(5, 1) == [5]
    assert cc.chunk_walk(1040, 520) == [[512, 8], [512, 8]] and cc.chunk_walk(700, 752) == [[512, 188]]
    assert cc.chunk_walk(300, 256) == [[256], [44]] and cc.chunk_walk(512, 512) == [[512]]


def test_new_cases_take_the_paths_they_were_made_for():
    """The numbers of the case table's last column, from the restatement."""
    h0, h1 = launches_of("H")[7]
    assert (h1.K, h1.KT, h1.fwd_S, h1.fwd_steps) == (144, 146, 4, (19, 18, 18, 18))
    assert (h1.k_tiles, h1.n_tiles, h1.out_map[2] % 32) == (5, 2, 1) and h1.below and h1.pads == (1, 1, 1, 1)
    assert not h0.dgrad and cc.CASES["H"].stem[0][4] == "tanh"
    i0, i1 = launches_of("I")[6]
    assert i1.below and i1.pads == (0, 1, 0, 1) and cc.CASES["I"].stem[0][4] == "relu"
    (j,) = launches_of("J")[33]
    assert (j.K, j.KT, j.fwd_S, j.k_tiles, j.M, j.fwd_tiles) == (4094, 4096, 4, 128, 33, 2)
    assert j.fwd_lds == 32768 + 4 * 4096 and j.fwd_lds <= 65536          # the tap table and the four waves' reduction beside it
    (k,) = launches_of("K")[5]
    assert k.kernel == (5, 5) and k.in_map == (2, 3, 2) and k.out_map == (2, 3, 3) and k.pads == (2, 2, 2, 2)
    a5, a130 = launches_of("a1")[5][0], launches_of("a1")[130][0]
    assert a130.rows_per_g == 520 and a130.G == 256 and set(a130.chunks) == {(512, 8)} and a130.wgrad_S == 4
    assert a5.G == 10 and a5.chunks[:9] == ((512, 8),) * 9 and a5.chunks[9] == (440,)
    (a2,) = launches_of("a2")[3]
    assert (a2.M, a2.rows_per_g, a2.G) == (2883, 752, 4) and a2.chunks == ((512, 240),) * 3 + ((512, 115),)
    (b,) = launches_of("b")[4097]
    assert b.M == cc.CONV_MAX_ROWS - 1 and b.G == 256 and all(len(r) == 128 for r in b.chunks) and b.chunks[-1][-1] == 511
    # every old case runs single-chunk ranges, the data gradient without `below` and unpadded: the gap the new rows close
    for name in cc.OLD:
        for ls in launches_of(name).values():
            for L in ls:
                assert all(len(r) == 1 for r in L.chunks) and not L.below and (not L.dgrad or not any(L.pads)), name
                assert not (L.k_tiles > 1 and L.n_tiles > 1) and L.K <= 72, name


# ---------------------------------------------------------------- the cases against the table of cells
def cells_by_name():
    by_cell = {}
    for name in EVERYTHING:
        for cell in cc.reached_cells(name):
            by_cell.setdefault(cell, []).append(name)
    return by_cell


def test_cases_reach_every_cell_and_each_new_one_is_needed():
    by_cell = cells_by_name()
    lost = sorted(cc.LAUNCH_CELLS - set(by_cell))
    assert not lost, f"cells no case reaches: {lost}"
    assert set(by_cell) == set(cc.LAUNCH_CELLS)
    for name in cc.NEW + tuple(cc.PATH_SHAPES):
        only = [cell for cell, names in by_cell.items() if names == [name]]
        print(name, "alone reaches", only)
        assert only, f"dropping {name} loses no cell"
        assert cc.OWNED[name] in only, (name, only)
    assert set(cc.OWNED) == set(cc.NEW) | set(cc.PATH_SHAPES)


@pytest.mark.parametrize("cell", sorted(cc.LAUNCH_CELLS))
def test_cell_is_reached(cell):
    assert any(cell in cc.reached_cells(name) for name in EVERYTHING), f"no case reaches the cell '{cell}'"


def test_launches_stay_inside_the_limits():
    """Every case and dedicated shape: LDS within 64 KiB, rows and indices within what pyz_stem_create admits."""
    for name in EVERYTHING:
        for ls in launches_of(name).values():
            for L in ls:
                assert L.fwd_lds <= 65536 and L.wgrad_lds <= 65536 and L.K <= cc.CONV_MAX_K and L.M <= cc.CONV_MAX_ROWS, name
                assert L.k_tiles * L.n_tiles * L.G < 2 ** 31 and L.M * L.out_map[2] < 2 ** 31, name
