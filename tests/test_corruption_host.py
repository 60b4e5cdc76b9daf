"""CPU checks of the corruption measures: the float64 restatements of tests/corruption_checks.py against independent
sources (scipy, PIL, colorsys) and known answers, the argument errors and declarations of pyz_corrupt_rows /
pyz_score_rows, the shares of elements the device tests leave open (on the very inputs those tests use), and the
bookkeeping of visualisations.Robustness over a stubbed BayesianModel.corruption_scores."""

import colorsys
import ctypes as C
import os
import re

import numpy as np
import pytest

import corruption_checks as cc
from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.visualisations import Robustness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1     # PYZ_E_INVALID, the library's code for a bad argument


# ---------------------------------------------------------------- the restatements against independent sources
@pytest.mark.parametrize("shape", [(3, 28, 28, 1), (2, 5, 7, 3), (2, 64, 64, 3)], ids=str)
def test_blur_equals_scipy_gaussian_filter(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    v = np.random.default_rng(1).random(shape)
    for sev in cc.SEVERITIES:
        sigma = float(cc.TABLE[cc.BLUR][sev - 1])
        mine = cc.blur_axis(cc.blur_axis(v, 1, sigma), 2, sigma)
        for i in range(shape[0]):
            for k in range(shape[3]):
                ref = ndimage.gaussian_filter(v[i, :, :, k], sigma=sigma, truncate=4.0, mode="nearest")
                assert np.abs(mine[i, :, :, k] - ref).max() <= 1e-12


@pytest.mark.parametrize("hw", [(8, 8), (5, 7), (28, 28), (64, 64), (11, 6)], ids=str)
def test_pixelate_is_within_one_grey_level_of_pil(hw):
    """PIL rounds to 8 bits between its two passes and at the end: one grey level.  The BOX pass alone is compared on every
    pixel.  Of the NEAREST pass the rows and columns whose source coordinate (i + 0.5) small / in is an exact integer
    (7 -> 4 at i = 3, 28 -> 16 at i = 3, 10, ...) are left out: PIL accumulates that coordinate by repeated addition and
    lands on either side of the integer, the restatement computes it in one rounding, as include/pyz.h states it."""
    Image = pytest.importorskip("PIL.Image")
    h, w = hw
    img = np.random.default_rng(2).integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    box = getattr(Image, "Resampling", Image).BOX
    nearest = getattr(Image, "Resampling", Image).NEAREST
    for sev in cc.SEVERITIES:
        c = cc.TABLE[cc.PIXELATE][sev - 1]
        oh, ow = cc.small_shape(h, w, c)
        small = Image.fromarray(img).resize((ow, oh), box)
        v = img[None].astype(np.float64)
        down = np.einsum("jh,nhik->njik", cc.box_weights(h, oh), np.einsum("iw,nhwk->nhik", cc.box_weights(w, ow), v))[0]
        assert np.abs(down - np.asarray(small, dtype=np.float64)).max() <= 1.0 + 1e-9, sev
        ref = np.asarray(small.resize((w, h), nearest), dtype=np.float64)
        mine = cc.pixelate(v, c)[0]
        rows = np.array([((2 * i + 1) * oh) % (2 * h) != 0 for i in range(h)])
        cols = np.array([((2 * i + 1) * ow) % (2 * w) != 0 for i in range(w)])
        assert rows.sum() >= h - oh and cols.sum() >= w - ow
        diff = np.abs(mine - ref)[rows][:, cols]
        assert diff.max() <= 1.0 + 1e-9, (sev, diff.max())


def test_hsv_round_trip_equals_colorsys():
    rng = np.random.default_rng(3)
    v = rng.integers(0, 256, size=(400, 3)) / 255.0
    v[:50, 1] = v[:50, 0]                    # ties between channels, and grey pixels
    v[50:80] = v[50:80, :1]
    H, S, V = cc.rgb2hsv(v)
    ref = np.array([colorsys.rgb_to_hsv(*p) for p in v])
    np.testing.assert_allclose(np.stack([H, S, V], axis=1), ref, atol=1e-14)
    back = cc.hsv2rgb(H, S, V)
    np.testing.assert_allclose(back, np.array([colorsys.hsv_to_rgb(*p) for p in ref]), atol=1e-14)
    np.testing.assert_allclose(back, v, atol=1e-14)


# ---------------------------------------------------------------- known answers
def test_contrast_of_a_constant_image_is_the_image():
    x = np.full((2, 6, 5, 3), 77.0)
    for sev in cc.SEVERITIES:
        np.testing.assert_allclose(cc.corrupt(x, cc.CONTRAST, sev, 255.0, 0)["value"], 77.0 / 255.0, atol=1e-15)


def test_brightness_and_saturate_of_a_grey_image():
    x = np.random.default_rng(4).integers(0, 256, size=(2, 4, 4, 1)).astype(np.float64)
    v = x / 255.0
    for sev in cc.SEVERITIES:
        c = cc.TABLE[cc.BRIGHT][sev - 1]
        np.testing.assert_allclose(cc.corrupt(x, cc.BRIGHT, sev, 255.0, 0)["value"], np.repeat(np.clip(v + c, 0, 1), 3, 3),
                                   atol=1e-15)
        s2 = np.clip(cc.TABLE[cc.SATURATE][sev - 1][1], 0, 1)
        got = cc.finish(cc.corrupt(x, cc.SATURATE, sev, 255.0, 0)["value"], 1, 1.0, False)
        np.testing.assert_allclose(got, (v * (1 - 2 * s2 / 3)).reshape(2, -1), atol=1e-15)


def test_impulse_noise_flips_a_binomial_share():
    x = np.full((4, 32, 32, 3), 128.0)
    for sev in cc.SEVERITIES:
        c = cc.TABLE[cc.IMPULSE][sev - 1]
        res = cc.corrupt(x, cc.IMPULSE, sev, 255.0, 11)
        n = res["flipped"].size
        assert abs(res["flipped"].mean() - c) <= 5 * np.sqrt(c * (1 - c) / n)
        salt = (res["value"][res["flipped"]] == 1.0).mean()
        assert abs(salt - 0.5) <= 5 * np.sqrt(0.25 / res["flipped"].sum())
        assert (res["value"][~res["flipped"]] == 128.0 / 255.0).all()


def test_impulse_thresholds_are_the_same_in_float32():
    """The kernel compares the fp32-exact uniforms (k + 0.5) 2^-23 with float32(c): no uniform lies between c and float32(c)."""
    for c in cc.TABLE[cc.IMPULSE] + [0.5]:
        assert np.floor(c * 2.0 ** 23 - 0.5) == np.floor(float(np.float32(c)) * 2.0 ** 23 - 0.5)
        assert c * 2.0 ** 23 - 0.5 != np.floor(c * 2.0 ** 23 - 0.5)


@pytest.mark.parametrize("lam", [0.3, 3.0, 12.0, 60.0])
def test_poisson_inversion_moments(lam):
    u, _ = cc.uniform_pairs(5, cc.SHOT, 1, 100_000)
    K, dist = cc.poisson_inversion(np.full(u.shape, lam), u)
    n = len(K)
    assert abs(K.mean() - lam) <= 5 * np.sqrt(lam / n)
    # var of the sample variance of a Poisson: (lam + 2 lam^2 (n / (n - 1))) / n
    assert abs(K.var(ddof=1) - lam) <= 5 * np.sqrt((lam + 2 * lam ** 2) / n)
    assert (dist >= 0).all()


def test_box_weights_and_nearest_indices():
    W = cc.box_weights(8, 4)
    assert (W == np.kron(np.eye(4), [[0.5, 0.5]])).all()
    assert (cc.box_weights(7, 1) == np.full((1, 7), 1 / 7)).all()
    assert list(cc.nearest_index(8, 4)) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert cc.small_shape(5, 7, 0.25) == (1, 1) and cc.small_shape(28, 28, 0.6) == (16, 16)
    for n_in, n_out in [(5, 3), (7, 4), (11, 6), (28, 16), (64, 19), (64, 38)]:
        W = cc.box_weights(n_in, n_out)
        np.testing.assert_allclose(W.sum(axis=1), 1.0)
        assert (W.sum(axis=0) > 0).all()                 # every source pixel counts somewhere


def test_finish_quantises_and_averages_like_the_reference():
    value = np.array([[[[0.2, 0.5, 1.0], [0.999, 0.0, 0.004]]]])
    assert cc.finish(value, 3, 255.0, True).tolist() == [[51.0, 127.0, 255.0, 254.0, 0.0, 1.0]]      # np.uint8 truncates
    np.testing.assert_allclose(cc.finish(value, 1, 255.0, True), [[(51 + 127 + 255) / 3, 255 / 3]])
    np.testing.assert_allclose(cc.finish(value, 1, 1.0, False), [[1.7 / 3, 1.003 / 3]])
    f32 = cc.finish(value, 1, 1.0, True, dtype=np.float32)
    assert f32.dtype == np.float32
    np.testing.assert_allclose(f32, cc.finish(value, 1, 1.0, True), rtol=1e-6)


# ---------------------------------------------------------------- what the device tests leave open
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_shot_noise_ambiguous_share_is_under_its_cap(case):
    """Elements whose uniform lies within AMBIGUOUS_EPS of a float64 CDF boundary, on the device tests' own inputs."""
    for pm in (255.0, 1.0):
        x = cc.case_input(case, pm)
        for sev in cc.SEVERITIES:
            dist = cc.corrupt(x, cc.SHOT, sev, pm, cc.SEED)["dist"]
            share = float((dist <= cc.AMBIGUOUS_EPS).mean())
            assert share <= cc.AMBIGUOUS_CAP, (sev, share)
            if case.ch == 1:                        # a grey output pixel is open if any of its three elements is
                assert float((dist <= cc.AMBIGUOUS_EPS).any(axis=-1).mean()) <= cc.AMBIGUOUS_CAP


def test_bounds_are_far_below_a_grey_level():
    """The derived float32 bounds leave the comparison sharp: every one is under a tenth of a grey level."""
    for case in cc.CASES:
        x = cc.case_input(case, 255.0)
        for kind in (cc.GAUSS, cc.SPECKLE, cc.BLUR, cc.CONTRAST, cc.BRIGHT, cc.SATURATE, cc.PIXELATE):
            for sev in cc.SEVERITIES:
                res = cc.corrupt(x, kind, sev, 255.0, cc.SEED)
                b = cc.bound(kind, sev, res, res["value"].shape)
                assert b.shape == res["value"].shape and (b > 0).all() and b.max() + cc.OUT_TAIL < 0.1 / 255.0, (kind, sev)


# ---------------------------------------------------------------- the C ABI
CTYPE = {"const float *": _lib._p, "const void *": _lib._p, "float *": _lib._p, "void *": _lib._p, "int": C.c_int,
         "float": _lib._f, "int64_t": _lib._i64, "uint64_t": _lib._u64, "const int32_t *": C.POINTER(_lib._i32)}


@pytest.mark.parametrize("name,count", [("pyz_corrupt_rows", 13), ("pyz_score_rows", 8)])
def test_entry_points_are_declared_with_matching_argument_types(name, count):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pyz.h")).read(), flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert proto, f"{name} is not declared in include/pyz.h"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    types = [re.sub(r"\s*\w+$", "", p) if not p.endswith("*") else p for p in params]
    types = [t if not t.endswith("*") else t[:-1].strip() + " *" for t in types]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int
    assert [CTYPE[t] for t in types] == list(argtypes) and len(argtypes) == count
    assert hasattr(_lib.load(), name)
    assert _lib.header_version() == 302
    api = open(os.path.join(ROOT, "bayesian_inference_for_nn_amd", "csrc", "pyz_api.hip")).read()
    assert '#include "pyz_corrupt.h"' in api
    rng = open(os.path.join(ROOT, "bayesian_inference_for_nn_amd", "csrc", "pyz_rng.h")).read()
    assert re.search(r"#define PYZ_STREAM_CORRUPT 7u", rng) and _lib.STREAM_CORRUPT == cc.STREAM_CORRUPT == 7


def _corrupt_rc(h=8, w=8, ch=1, kind=0, sev=(1,), n_sev=None, n=1):
    lib = _lib.load()
    arr = (C.c_int32 * max(1, len(sev)))(*sev)
    rc = lib.pyz_corrupt_rows(None, n, h, w, ch, kind, arr, len(sev) if n_sev is None else n_sev, 255.0, 1, 0, None, None)
    return rc, lib.pyz_last_error().decode()


def test_argument_errors_need_no_gpu():
    for kw, word in ((dict(ch=2), "channels"), (dict(sev=(0,)), "severity"), (dict(sev=(1, 6)), "severity"),
                     (dict(kind=10), "kind"), (dict(kind=-1), "kind"), (dict(h=200, w=200), "LDS"),
                     (dict(sev=(1, 2, 3, 4, 5, 5)), "n_sev"), (dict(n_sev=0), "n_sev"), (dict(n=0), "positive"),
                     (dict(kind=9, h=2), "h = ch = 1"), (dict(h=83, w=82, ch=3), "LDS")):
        rc, msg = _corrupt_rc(**kw)
        assert rc == E_INVALID and word in msg, (kw, rc, msg)
    # valid shapes get as far as the pointer check: 64 x 64 x 3 fits (82 x 82 is the largest square), a long row is no image
    for kw in (dict(h=64, w=64, ch=3, kind=4), dict(h=82, w=82, ch=3, kind=8), dict(kind=9, h=1, w=100000, ch=1)):
        rc, msg = _corrupt_rc(**kw)
        assert rc == E_INVALID and "null device pointer" in msg, (kw, msg)
    lib = _lib.load()
    for args, word in (((None, 1, 5, 3, None, 2, None, None), "kind"), ((None, 0, 5, 3, None, 0, None, None), "positive"),
                       ((None, 1, 5, 0, None, 1, None, None), "positive"), ((None, 1, 5, 3, None, 0, None, None), "null")):
        assert lib.pyz_score_rows(*args) == E_INVALID and word in lib.pyz_last_error().decode(), args


# ---------------------------------------------------------------- Robustness over a stubbed model
class _Split:
    def __init__(self, x, y):
        self._xy = (x, y)

    def as_numpy(self):
        return self._xy


class _Data:
    def __init__(self, x, y, regression=False):
        self.likelihood_model = "Regression" if regression else "Classification"
        self.valid_data = _Split(x, y)


class _Stub:
    """corruption_scores returns fixed numbers per kind and records its calls; predictive_mean is right on all rows but
    `wrong_clean` (classification) or off by 0.5 everywhere (regression)."""

    def __init__(self, y, wrong_clean=3):
        self.calls = []
        self.y = np.asarray(y)
        self.wrong_clean = wrong_clean

    def fractions(self, kind):
        return np.array([0.1, 0.2, 0.3, 0.4, 0.5]) * (kind + 1) / 10.0

    def corruption_scores(self, x, y, image_shape, kind, severities, nb_samples, regression, pixel_max, seed):
        self.calls.append(dict(shape=tuple(image_shape), kind=kind, severities=list(severities), nb_samples=nb_samples,
                               regression=regression, pixel_max=pixel_max, seed=seed))
        return self.fractions(kind) * (10.0 if regression else 1.0)

    def predictive_mean(self, x, nb_samples):
        if self.y.dtype.kind == "f":
            return (self.y + 0.5).astype(np.float32)
        p = np.zeros((len(self.y), 4), dtype=np.float32)
        p[np.arange(len(self.y)), self.y] = 1.0
        p[:self.wrong_clean] = np.roll(p[:self.wrong_clean], 1, axis=1)
        return p


def _classification(shape=(20, 6, 6)):
    y = np.arange(20) % 4
    stub = _Stub(y)
    return stub, Robustness(stub, _Data(np.zeros(shape, np.float32), y), seed=9)


def test_attributes_follow_the_reference():
    stub, rb = _classification()
    assert tuple(rb.corruptions) == cc.NAMES and rb.corruption_dict == {n: k for k, n in enumerate(cc.NAMES)}
    assert rb.error_dict == {n: None for n in cc.NAMES} and list(rb.severities) == [1, 2, 3, 4, 5]
    assert rb.pixel_max == 255.0 and rb.seed == 9
    a, b = Robustness(stub, rb.dataset).seed, Robustness(stub, rb.dataset).seed
    assert a != b                                             # seed=None: a fresh seed at construction
    assert Robustness(stub, rb.dataset, pixel_max=1.0, seed=4).pixel_max == 1.0


def test_corruption_error_absolute_and_relative(capsys):
    stub, rb = _classification()
    fr = stub.fractions(5)
    v = rb.corruption_error("contrast", nb_boundaries=7)
    assert v == pytest.approx(np.sum(fr * 100) / 5)
    assert capsys.readouterr().out == "Corruption Error for contrast: {}%\n".format(v)
    assert stub.calls == [dict(shape=(6, 6, 1), kind=5, severities=[1, 2, 3, 4, 5], nb_samples=7, regression=False,
                               pixel_max=255.0, seed=9)]
    clean = 3 / 20                                            # a FRACTION, subtracted from the percentages (:191-192)
    r = rb.corruption_error("contrast", relative=True)
    assert r == pytest.approx(np.sum(fr * 100 - clean) / 5)
    assert capsys.readouterr().out == "Relative Error for contrast: {}%\n".format(r)
    assert rb.corruption_error("contrast", helper=True) == v and capsys.readouterr().out == ""
    assert len(stub.calls) == 1
    with pytest.raises(KeyError):
        rb.corruption_error("fog")


def test_mean_corruption_error_and_the_cache_in_any_order(capsys, tmp_path):
    stub, rb = _classification((20, 6, 6, 3))
    sev = rb.corruption_robustness_by_severity("pixelate", nb_samples=5, save_path=str(tmp_path))
    np.testing.assert_allclose(sev, stub.fractions(8) * 100)
    assert (tmp_path / "report" / "robustness" / "figures" / "corruption_robustness_by_severity.png").exists() or \
        "matplotlib unavailable" in capsys.readouterr().out
    nine = rb.robustness_by_corruption(save_path=str(tmp_path))
    assert nine.shape == (9,)
    np.testing.assert_allclose(nine, [np.sum(stub.fractions(k) * 100) / 5 for k in range(9)])
    capsys.readouterr()
    m = rb.mean_corruption_error()
    assert m == pytest.approx(np.mean(nine)) and capsys.readouterr().out == "Mean Corruption Error: " + str(m) + " %\n"
    mr = rb.mean_corruption_error(relative=True, save_path=str(tmp_path))
    assert mr == pytest.approx(np.mean(nine) - 3 / 20)
    assert (tmp_path / "report" / "robustness" / "mean_relative_error.txt").read_text() == str(mr)
    rb.mean_corruption_error(save_path=str(tmp_path))
    assert (tmp_path / "report" / "robustness" / "mean_corruption_error.txt").read_text() == str(m)
    rb.corruption_error("shot_noise", save_path=str(tmp_path))
    rb.corruption_error("shot_noise", relative=True, save_path=str(tmp_path))
    assert (tmp_path / "report" / "robustness" / "corruption_error_shot_noise.txt").read_text() == \
        str(np.sum(stub.fractions(1) * 100) / 5)
    assert (tmp_path / "report" / "robustness" / "relative_error_shot_noise.txt").exists()
    # one read-out per corruption, whatever was called first; the shape of a colour split
    assert sorted(c["kind"] for c in stub.calls) == list(range(9))
    assert all(c["shape"] == (6, 6, 3) for c in stub.calls)
    for name, kind in rb.corruption_dict.items():
        np.testing.assert_array_equal(rb.error_dict[name], stub.fractions(kind))      # fractions, whoever filled it


def test_regression_branch(capsys):
    y = np.linspace(-1, 1, 12).reshape(12, 1).astype(np.float32)
    stub = _Stub(y)
    rb = Robustness(stub, _Data(np.zeros((12, 7), np.float32), y, regression=True), seed=2)
    rmse = stub.fractions(9) * 10.0
    v = rb.corruption_error("contrast", helper=True)           # the name is ignored (:181)
    assert v == pytest.approx(rmse.sum() / 5)
    assert stub.calls[0]["kind"] == 9 and stub.calls[0]["shape"] == (1, 7, 1) and stub.calls[0]["regression"] is True
    m = rb.mean_corruption_error(relative=True)
    assert m == pytest.approx(np.sum(rmse - 0.5) / 5)          # the clean RMSE of the stub is 0.5
    assert capsys.readouterr().out == "Mean Relative Error: " + str(m) + "\n"
    np.testing.assert_allclose(rb.corruption_robustness_by_severity(), rmse)


def test_a_split_that_holds_no_images_is_refused():
    y = np.arange(20) % 4
    for shape in ((20, 36), (20, 6, 6, 2), (20, 2, 3, 3, 3)):
        rb = Robustness(_Stub(y), _Data(np.zeros(shape, np.float32), y), seed=1)
        with pytest.raises(ValueError, match=re.escape(str(shape[1:]))):
            rb.corruption_error("contrast", helper=True)
