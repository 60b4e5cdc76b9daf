"""Float64 restatements behind the tests of pyz_corrupt_rows / pyz_score_rows and of Robustness's corruption measures:

* the ten corruption kinds of include/pyz.h (the reference functions of Pyesian/visualisations/Robustness.py:10-93 without
  PIL or skimage), on the library's Philox stream PYZ_STREAM_CORRUPT restated by oracle/philox.py;
* ``finish``: the quantisation, channel mean and scaling of the output;
* ``bound``: per-element float32 error bounds of the kernel's arithmetic, DERIVED (below), not measured;
* ``CASES`` / ``ROW_CASES``: the case tables of tests/test_gpu_corruption.py and tests/test_corruption_host.py."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import philox as o_philox

STREAM_CORRUPT = 7
NAMES = ("gaussian_noise", "shot_noise", "impulse_noise", "speckle_noise", "gaussian_blur", "contrast", "brightness",
         "saturate", "pixelate")
GAUSS, SHOT, IMPULSE, SPECKLE, BLUR, CONTRAST, BRIGHT, SATURATE, PIXELATE, REGRESSION = range(10)
# Robustness.py:11,22,29,35,41,47,54,68,85 and :17
TABLE = {GAUSS: [.08, .12, 0.18, 0.26, 0.38], SHOT: [60, 25, 12, 5, 3], IMPULSE: [.03, .06, .09, 0.17, 0.27],
         SPECKLE: [.15, .2, 0.35, 0.45, 0.6], BLUR: [1, 2, 3, 4, 6], CONTRAST: [0.4, .3, .2, .1, .05],
         BRIGHT: [.1, .2, .3, .4, .5], SATURATE: [(0.3, 0), (0.1, 0), (2, 0), (5, 0.1), (20, 0.2)],
         PIXELATE: [0.6, 0.5, 0.4, 0.3, 0.25], REGRESSION: [.08, .12, 0.18, 0.26, 0.38]}
SEVERITIES = (1, 2, 3, 4, 5)
U = 2.0 ** -24                                    # float32 unit roundoff
R_MAX = float(np.sqrt(48 * np.log(2.0)))          # the largest Box-Muller radius: u >= 2^-24


def step(kind, severity):
    return 8 * kind + severity


def clip(a):
    return np.clip(a, 0.0, 1.0)


def replicate(x, pixel_max):
    """x (n, h, w, ch) -> v (n, h, w, 3) float64 in units of pixel_max (Robustness.py:260-266)."""
    v = np.asarray(x, dtype=np.float64) / float(pixel_max)
    return np.repeat(v, 3, axis=3) if v.shape[3] == 1 else v


def normals(seed, kind, severity, count):
    return o_philox.normal(seed, STREAM_CORRUPT, step(kind, severity), count)


def uniform_pairs(seed, kind, severity, count):
    """(u0, u1) of the elements 0 .. count - 1: words x and y of the counter idx4 = e."""
    w = o_philox.words(seed, STREAM_CORRUPT, step(kind, severity), 4 * count).reshape(count, 4)
    unit = lambda a: ((a >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    return unit(w[:, 0]), unit(w[:, 1])


# ---------------------------------------------------------------- the kinds
def poisson_inversion(lam, u):
    """(K, distance of u to the nearest CDF boundary): p = exp(-lam); s = p; k = 0; while (u > s && k < 255) {...}."""
    lam, u = np.asarray(lam, dtype=np.float64), np.asarray(u, dtype=np.float64)
    p = np.exp(-lam)
    s = p.copy()
    k = np.zeros(lam.shape, dtype=np.int64)
    below = np.full(lam.shape, -np.inf)
    active = (u > s) & (k < 255)
    while active.any():
        below[active] = s[active]
        k[active] += 1
        p[active] *= lam[active] / k[active]
        s[active] += p[active]
        active = (u > s) & (k < 255)
    return k, np.minimum(u - below, np.abs(s - u))


def blur_axis(a, axis, sigma):
    r = int(4 * sigma + 0.5)
    k = np.arange(-r, r + 1)
    wt = np.exp(-0.5 * k.astype(np.float64) ** 2 / sigma ** 2)
    wt = wt / wt.sum()
    L = a.shape[axis]
    out = np.zeros_like(a)
    for t, wk in zip(k, wt):
        out = out + wk * np.take(a, np.clip(np.arange(L) + t, 0, L - 1), axis=axis)
    return out


def box_weights(n_in, n_out):
    """(n_out, n_in) normalised BOX weights along one axis."""
    W = np.zeros((n_out, n_in))
    scale = n_in / n_out
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo, hi = max(0, int(center - scale / 2 + 0.5)), min(n_in, int(center + scale / 2 + 0.5))
        for j in range(lo, hi):
            t = (j - center + 0.5) / scale
            if -0.5 < t <= 0.5:
                W[i, j] = 1.0
        W[i] /= W[i].sum()
    return W


def nearest_index(n_in, small):
    return np.array([min(small - 1, int(((i + 0.5) * small) / n_in)) for i in range(n_in)])


def small_shape(h, w, c):
    return max(1, int(h * c)), max(1, int(w * c))


def pixelate(v, c):
    n, h, w, _ = v.shape
    oh, ow = small_shape(h, w, c)
    a = np.einsum("iw,nhwk->nhik", box_weights(w, ow), v)        # horizontal pass first
    a = np.einsum("jh,nhik->njik", box_weights(h, oh), a)
    return a[:, nearest_index(h, oh)][:, :, nearest_index(w, ow)]


def rgb2hsv(v):
    """skimage.color.rgb2hsv's formulas."""
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    V = v.max(axis=-1)
    d = V - v.min(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(d == 0.0, 0.0, d / V)
        H = (g - b) / d                                            # red, green, blue assigned in turn: the last maximum wins
        H = np.where(g == V, 2.0 + (b - r) / d, H)
        H = np.where(b == V, 4.0 + (r - g) / d, H)
        H = np.where(d == 0.0, 0.0, np.mod(H / 6.0, 1.0))
    return H, S, V


def hsv2rgb(H, S, V):
    """skimage.color.hsv2rgb's formulas."""
    hi = np.floor(H * 6.0)
    f = H * 6.0 - hi
    p, q, t = V * (1 - S), V * (1 - f * S), V * (1 - (1 - f) * S)
    hi = hi.astype(np.int64) % 6
    return np.stack([np.choose(hi, [V, q, p, p, t, V]), np.choose(hi, [t, V, V, q, p, p]),
                     np.choose(hi, [p, p, t, V, V, q])], axis=-1)


def corrupt(x, kind, severity, pixel_max, seed):
    """x (n, h, w, ch) -> dict(value=(n, h, w, 3) float64 in [0, 1] before the quantisation, plus what the bounds and the
    exactness tests need: z (normals), flipped (impulse), dist (shot: distance of u to the nearest CDF boundary)."""
    c = TABLE[kind][severity - 1]
    v = replicate(x, pixel_max)
    count = v.size
    out = {}
    if kind in (GAUSS, SPECKLE):
        z = normals(seed, kind, severity, count).reshape(v.shape)
        out["z"] = z
        out["value"] = clip(v + c * z) if kind == GAUSS else clip(v + v * c * z)
    elif kind == SHOT:
        u, _ = uniform_pairs(seed, kind, severity, count)
        K, dist = poisson_inversion(clip(v) * c, u.reshape(v.shape))
        out["dist"] = dist
        out["value"] = clip(K / float(c))
    elif kind == IMPULSE:
        u0, u1 = (a.reshape(v.shape) for a in uniform_pairs(seed, kind, severity, count))
        out["flipped"] = u0 < c
        out["value"] = clip(np.where(u0 < c, np.where(u1 < 0.5, 1.0, 0.0), v))
    elif kind == BLUR:
        out["value"] = clip(blur_axis(blur_axis(v, 1, float(c)), 2, float(c)))
    elif kind == CONTRAST:
        m = v.mean(axis=(1, 2), keepdims=True)
        out["value"] = clip((v - m) * c + m)
    elif kind in (BRIGHT, SATURATE):
        H, S, V = rgb2hsv(v)
        out["hsv"] = (H, S, V)
        if kind == BRIGHT:
            V2, S2 = clip(V + c), S
        else:
            V2, S2 = V, clip(S * c[0] + c[1])
        out["hsv2"] = (H, S2, V2)
        out["value"] = clip(hsv2rgb(H, S2, V2))
    elif kind == PIXELATE:
        out["value"] = clip(pixelate(v, c))
    else:
        raise ValueError(kind)
    return out


def regression_noise(x, severity, seed):
    """x (n, L) -> (x + c z, z)."""
    x = np.asarray(x, dtype=np.float64)
    z = normals(seed, REGRESSION, severity, x.size).reshape(x.shape)
    return x + TABLE[REGRESSION][severity - 1] * z, z


def finish(value, ch, pixel_max, quantise, dtype=np.float64):
    """value (n, h, w, 3) in [0, 1] -> (n, h * w * ch) output rows.  dtype float32: the kernel's own operations in its own
    order (floor(255 v), (a + b + c) / 3, times pixel_max / 255 or pixel_max), bit for bit."""
    f = dtype
    value = np.asarray(value, dtype=f)
    scale = f(pixel_max)
    if quantise:
        value = np.floor(f(255.0) * value)
        scale = f(pixel_max) / f(255.0)
    if ch == 1:
        value = ((value[..., 0] + value[..., 1] + value[..., 2]) / f(3.0))[..., None]
    return (value * scale).astype(f).reshape(len(value), -1)


# ---------------------------------------------------------------- float32 error bounds (derived)
def normal_err(z):
    """|device normal - float64 normal| for the same Philox words.  z = r cos / sin(2 pi u_b), r = sqrt(-2 ln u_a).  The
    device library documents logf and sincospif at <= 2 ulp, sqrt and the products are correctly rounded: ln u_a is off by
    <= 2 * 2^-23 relative, the square root halves that and adds 2^-24 (r: <= 2 * 2^-23 relative, with the final product
    2.5 * 2^-23); the trigonometric factor is off by <= 2 ulp(1) = 2 * 2^-23 absolute, times r <= R_MAX."""
    return (2.5 * np.abs(z) + 2.0 * R_MAX) * 2.0 ** -23


def bound(kind, severity, res, shape, x=None):
    """Per-element bound (n, h, w, 3) on |float32 kernel value - float64 value| in [0, 1] units, before the output
    stage.  Every float32 operation rounds to within U = 2^-24 relative; the input v = x / pixel_max carries U; clip is
    1-Lipschitz.  res = corrupt(...)."""
    c = TABLE[kind][severity - 1]
    n, h, w, _ = shape
    val = res["value"]
    one = np.ones(val.shape)
    if kind == GAUSS:       # v + c z: input U, product and sum (or their fusion) 2 roundings, the normal's own error times c
        az = np.abs(res["z"])
        return U * (2.0 + 2.0 * c * az) + c * normal_err(res["z"])
    if kind == SPECKLE:     # v + v c z: input U (1 + c |z|), three roundings on terms <= 1 + c |z|
        az = np.abs(res["z"])
        return U * (2.0 + 4.0 * c * az) + c * normal_err(res["z"])
    if kind == BLUR:        # per pass 2r + 1 fused multiply-adds and the rounded weight: (2r + 2) U on sums <= 1; input U
        r = int(4 * c + 0.5)
        return U * (2 * (2 * r + 2) + 1) * one
    if kind == CONTRAST:    # m: ceil(hw / 256) sequential terms per thread, an 8-level tree, a division, the input; then
        return U * (-(-h * w // 256) + 16) * one     # (v - m) c + m: three roundings and (1 + c) dm + c dv <= 4 more
    if kind == PIXELATE:    # per pass a sum of <= ceil(scale) + 1 terms and a division; input U
        oh, ow = small_shape(h, w, c)
        return U * (1 + (-(-w // ow) + 2) + (-(-h // oh) + 2)) * one
    if kind in (BRIGHT, SATURATE):
        # d = max - min carries 3 U absolute (two inputs, one rounding): S = d / V is off by 4 U / V, S' by c0 times that
        # (saturate); the hue's ratio (a - b) / d by 6 U / d and 6 h, its fraction f, by (6 / d + 20) U.  The outputs are
        # V' (1 - S'), V' (1 - f S'), V' (1 - (1 - f) S'): V' (dS' + S' df), and 64 U for V's own error and the dozen
        # roundings on values <= 1.  d = 0: h = f = S = 0 exactly in both precisions.
        H, S, V = res["hsv"]
        _, S2, V2 = res["hsv2"]
        d = S * V
        amp = float(c[0]) if kind == SATURATE else 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            extra = np.where(d > 0, V2 * (amp * 4.0 / V + S2 * (6.0 / d + 20.0)), 0.0)
        return (U * (64.0 + extra))[..., None] * one
    raise ValueError(kind)


OUT_TAIL = 5 * U       # the output stage on values <= 1: two sums and a division of the channel mean, the scaling, and slack


def regression_bound(x, severity, z):
    """x + c z: the product and the sum round once each (or fuse); the normal's own error times c."""
    c = TABLE[REGRESSION][severity - 1]
    x = np.abs(np.asarray(x, dtype=np.float64))
    return U * (c * np.abs(z) + x + c * np.abs(z)) + c * normal_err(z)


AMBIGUOUS_EPS = 1e-5    # shot noise: an element whose u lies this close to a float64 CDF boundary may differ by one count
AMBIGUOUS_CAP = 0.005   # ... and at most this share of a case's elements may


# ---------------------------------------------------------------- case tables
class Case(NamedTuple):
    name: str
    h: int
    w: int
    ch: int
    n: int


CASES = [Case("8x8x1_n1", 8, 8, 1, 1), Case("8x8x1_n5", 8, 8, 1, 5), Case("8x8x3_n3", 8, 8, 3, 3),
         Case("5x7x3_n5", 5, 7, 3, 5), Case("5x7x3_n1", 5, 7, 3, 1), Case("28x28x1_n3", 28, 28, 1, 3),
         Case("64x64x3_n2", 64, 64, 3, 2)]
ROW_CASES = [(5, 11), (1, 1), (3, 13)]      # kind 9: (rows, length)
SEED = 20240607


def case_pixels(case: Case):
    """(n, h, w, ch) float32 integer pixel values 0..255."""
    rng = np.random.default_rng(500 + CASES.index(case))
    return rng.integers(0, 256, size=(case.n, case.h, case.w, case.ch)).astype(np.float32)


def row_case_data(rows, length):
    rng = np.random.default_rng(900 + 31 * rows + length)
    return rng.normal(size=(rows, length)).astype(np.float32)


def case_input(case: Case, pixel_max):
    """pixel_max 255: the integer pixels; pixel_max 1: the same values / 255 in float32."""
    x = case_pixels(case)
    return x if pixel_max == 255.0 else (x / np.float32(255.0)).astype(np.float32)
