// pyz_corrupt.h -- the image corruptions of the robustness measures and the scoring of their read-outs.
//
// Replaces the per-image Python loop through PIL and skimage of Robustness._error_rate / _corrupt and the nine
// corruption functions (Pyesian/visualisations/Robustness.py:10-93,235-273), and the sklearn scoring behind them
// (:250-254).  The semantics are the reference functions restated without PIL or skimage (include/pyz.h lists them).
//
// k_corrupt_rows: one workgroup of 256 threads per (image, severity); one launch covers every listed severity.
// The noise kinds and the two HSV kinds are pointwise: a thread reads its pixel from HBM and writes the result.  Blur,
// contrast and pixelate stage the image in LDS as PLANAR channels, A[k][y * w + x], beside a scratch copy B of the same
// size, and never read HBM again.  A grey image is staged as ONE plane: its three replicated channels are the same
// numbers through every deterministic kind, and the write-out replicates the value.
//
// LDS addressing.  Threads own consecutive pixels p = y * w + x of a dense plane (row pitch w, no pad), so in BOTH blur
// passes the 32 lanes of a group read A[p + k * w] or A[p + k]: 32 consecutive dwords, one per bank, whatever w is.  A
// padded pitch would break that (the lanes of a group span several rows when w < 32: rows y and y + 1 would then meet on a
// bank).  Clamped taps at the border collapse lanes onto the same address (a broadcast) or onto distinct columns of one
// row (distinct banks).  The pixelate passes read runs of a few source pixels per thread (stride = the scale, 1.7 to 4
// dwords: at most 4 lanes on a bank) over an image that is read once per pass.
//
// Noise: stream PYZ_STREAM_CORRUPT, step = 8 * kind + severity, element e = ((i h + y) w + x) 3 + k of the replicated
// three-channel tensor (kind 9: e = i w + j); a function of (seed, kind, severity, element) alone.
//
// k_score_rows: per group of n rows, the rows whose predicted class differs from the label (one integer atomic per
// wave) or, for regression, per-block float64 sums of squared errors that k_score_sum adds in block order.
#pragma once

#include <algorithm>
#include <cmath>

#include "pyz_common.h"
#include "pyz_rng.h"

#define PYZ_CORRUPT_THREADS 256
#define PYZ_CORRUPT_MAX_SEV 5
#define PYZ_CORRUPT_KINDS 10
#define PYZ_CORRUPT_REGRESSION 9
#define PYZ_CORRUPT_MAX_R 24       // int(4 * 6 + 0.5): the blur radius of severity 5
#define PYZ_LDS_BYTES (160 * 1024)

enum { PYZ_C_GAUSS = 0, PYZ_C_SHOT, PYZ_C_IMPULSE, PYZ_C_SPECKLE, PYZ_C_BLUR, PYZ_C_CONTRAST, PYZ_C_BRIGHT, PYZ_C_SATURATE,
       PYZ_C_PIXELATE };

// the reference's tables (Robustness.py:11,17,22,29,35,41,47,54,68,85), [kind][severity - 1]; saturate's second entry apart
static const double PYZ_CORRUPT_C[PYZ_CORRUPT_KINDS][5] = {
    {.08, .12, 0.18, 0.26, 0.38}, {60, 25, 12, 5, 3},       {.03, .06, .09, 0.17, 0.27}, {.15, .2, 0.35, 0.45, 0.6},
    {1, 2, 3, 4, 6},              {0.4, .3, .2, .1, .05},   {.1, .2, .3, .4, .5},        {0.3, 0.1, 2, 5, 20},
    {0.6, 0.5, 0.4, 0.3, 0.25},   {.08, .12, 0.18, 0.26, 0.38}};
static const double PYZ_SATURATE_C1[5] = {0, 0, 0, 0.1, 0.2};

struct CorruptArgs {
  const float *x;   // (n, h, w, ch)
  float *out;       // (n_sev, n, h, w, ch)
  long long n;
  int h, w, ch, kind;
  int planes;                              // channels staged in LDS: ch (a grey image's three are one)
  int sev[PYZ_CORRUPT_MAX_SEV];
  float c0[PYZ_CORRUPT_MAX_SEV], c1[PYZ_CORRUPT_MAX_SEV];
  int r[PYZ_CORRUPT_MAX_SEV];                          // blur: radius
  float bw[PYZ_CORRUPT_MAX_SEV][PYZ_CORRUPT_MAX_R + 1];   // blur: float32 of the normalised float64 weights, k = 0 .. r
  int oh[PYZ_CORRUPT_MAX_SEV], ow[PYZ_CORRUPT_MAX_SEV];   // pixelate: the small image
  float pixel_max;
  float out_scale;                         // quantise: pixel_max / 255 (float32 division), else pixel_max
  int quantise;
  uint64_t seed;
};

__device__ __forceinline__ float pyz_clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// skimage.color.rgb2hsv: the channels are assigned red, green, blue, so the LAST maximum wins a tie
__device__ __forceinline__ void pyz_rgb2hsv(float r, float g, float b, float &h, float &s, float &v) {
  v = fmaxf(r, fmaxf(g, b));
  const float d = v - fminf(r, fminf(g, b));
  float hh = (g - b) / d;
  if (g == v) hh = 2.0f + (b - r) / d;
  if (b == v) hh = 4.0f + (r - g) / d;
  hh = hh / 6.0f;
  hh = hh - floorf(hh);   // % 1
  h = d == 0.0f ? 0.0f : hh;
  s = d == 0.0f ? 0.0f : d / v;
}

// skimage.color.hsv2rgb
__device__ __forceinline__ void pyz_hsv2rgb(float h, float s, float v, float &r, float &g, float &b) {
  const float h6 = h * 6.0f, fl = floorf(h6), f = h6 - fl;
  const float p = v * (1.0f - s), q = v * (1.0f - f * s), t = v * (1.0f - (1.0f - f) * s);
  const int hi = (int)fl % 6;
  r = hi == 0 || hi == 5 ? v : (hi == 1 ? q : (hi == 4 ? t : p));
  g = hi == 1 || hi == 2 ? v : (hi == 0 ? t : (hi == 3 ? q : p));
  b = hi == 3 || hi == 4 ? v : (hi == 2 ? t : (hi == 5 ? q : p));
}

// K ~ Poisson(lam) by inversion from one uniform
__device__ __forceinline__ float pyz_poisson_inv(float lam, float u) {
  float p = expf(-lam), s = p;
  int k = 0;
  while (u > s && k < 255) {
    ++k;
    p *= lam / (float)k;
    s += p;
  }
  return (float)k;
}

// the three channel values in [0, 1] of pixel p -> the output row o (np.uint8 at Robustness.py:270, the channel mean at :246)
__device__ __forceinline__ void pyz_corrupt_emit(const CorruptArgs &g, float *o, int p, float a, float b, float c) {
  if (g.quantise) {
    a = floorf(255.0f * a);
    b = floorf(255.0f * b);
    c = floorf(255.0f * c);
  }
  if (g.ch == 1) {
    o[p] = (a + b + c) / 3.0f * g.out_scale;
  } else {
    o[3 * p + 0] = a * g.out_scale;
    o[3 * p + 1] = b * g.out_scale;
    o[3 * p + 2] = c * g.out_scale;
  }
}

// PIL's BOX coefficients along one axis (Resample.c precompute_coeffs, restated in include/pyz.h): the first and one past
// the last source index of weight 1 for output index i.  float64, uncontracted: the comparisons sit on exact halves for
// some sizes (11 -> 6 pixels), where the float64 restatement of the tests must see the same operations.
__device__ __forceinline__ int2 pyz_box_taps(int i, int in, int out) {
#pragma clang fp contract(off)
  const double scale = (double)in / (double)out, center = ((double)i + 0.5) * scale;
  const int lo = max(0, (int)(center - scale / 2.0 + 0.5)), hi = min(in, (int)(center + scale / 2.0 + 0.5));
  int j0 = hi, j1 = lo;
  for (int j = lo; j < hi; ++j) {
    const double t = ((double)j - center + 0.5) / scale;
    if (-0.5 < t && t <= 0.5) {
      j0 = min(j0, j);
      j1 = max(j1, j + 1);
    }
  }
  return make_int2(j0, j1);
}

// NEAREST: the source index of output index i
__device__ __forceinline__ int pyz_nearest_src(int i, int in, int small) {
#pragma clang fp contract(off)
  return min(small - 1, (int)((((double)i + 0.5) * (double)small) / (double)in));
}

__global__ void __launch_bounds__(PYZ_CORRUPT_THREADS) k_corrupt_rows(CorruptArgs g) {
  extern __shared__ __attribute__((aligned(16))) float cr_lds[];
  const int tid = threadIdx.x, s = blockIdx.y;
  const long long i = blockIdx.x;
  const int h = g.h, w = g.w, ch = g.ch, hw = h * w, kind = g.kind;
  const float c = g.c0[s], pm = g.pixel_max;
  const uint32_t step = 8u * (uint32_t)kind + (uint32_t)g.sev[s];
  const float *xi = g.x + i * (long long)hw * ch;
  float *o = g.out + ((long long)s * g.n + i) * (long long)hw * ch;

  if (kind == PYZ_CORRUPT_REGRESSION) {   // x + c z on every element of the row (Robustness.py:16-19,272-273)
    for (int j = tid; j < w; j += PYZ_CORRUPT_THREADS)
      o[j] = xi[j] + c * pyz_normal1(g.seed, PYZ_STREAM_CORRUPT, step, (uint64_t)i * (uint64_t)w + (uint64_t)j);
    return;
  }

  if (kind != PYZ_C_BLUR && kind != PYZ_C_CONTRAST && kind != PYZ_C_PIXELATE) {   // pointwise
    const float c1 = g.c1[s];
    const uint2 key = make_uint2((uint32_t)g.seed, (uint32_t)(g.seed >> 32));
    for (int p = tid; p < hw; p += PYZ_CORRUPT_THREADS) {
      float v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = xi[p * ch + (ch == 3 ? k : 0)] / pm;
      const uint64_t e0 = ((uint64_t)i * (uint64_t)hw + (uint64_t)p) * 3u;
      if (kind == PYZ_C_GAUSS || kind == PYZ_C_SPECKLE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float z = pyz_normal1(g.seed, PYZ_STREAM_CORRUPT, step, e0 + k);
          v[k] = pyz_clip01(kind == PYZ_C_GAUSS ? v[k] + c * z : v[k] + v[k] * c * z);
        }
      } else if (kind == PYZ_C_SHOT || kind == PYZ_C_IMPULSE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const uint64_t e = e0 + k;   // a counter of its own per element: word x = u / u0, word y = u1
          const uint4 rw = philox4x32_10(make_uint4((uint32_t)e, (uint32_t)(e >> 32), step, PYZ_STREAM_CORRUPT), key);
          const float u0 = pyz_unit(rw.x), u1 = pyz_unit(rw.y);
          if (kind == PYZ_C_SHOT) v[k] = pyz_clip01(pyz_poisson_inv(pyz_clip01(v[k]) * c, u0) / c);
          else v[k] = pyz_clip01(u0 < c ? (u1 < 0.5f ? 1.0f : 0.0f) : v[k]);   // skimage 's&p', salt_vs_pepper = 0.5
        }
      } else {   // brightness / saturate through HSV
        float hh, ss, vv;
        pyz_rgb2hsv(v[0], v[1], v[2], hh, ss, vv);
        if (kind == PYZ_C_BRIGHT) vv = pyz_clip01(vv + c);
        else ss = pyz_clip01(ss * c + c1);
        pyz_hsv2rgb(hh, ss, vv, v[0], v[1], v[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = pyz_clip01(v[k]);
      }
      pyz_corrupt_emit(g, o, p, v[0], v[1], v[2]);
    }
    return;
  }

  // ---- the staged kinds: red[256] | A[planes][hw] | B[planes][hw] | pixelate's tap table
  const int planes = g.planes;
  float *red = cr_lds, *A = cr_lds + PYZ_CORRUPT_THREADS, *B = A + planes * hw;
  for (int p = tid; p < hw; p += PYZ_CORRUPT_THREADS)
    for (int k = 0; k < planes; ++k) A[k * hw + p] = xi[p * ch + k] / pm;
  __syncthreads();
  const float *res = A;   // where the result planes stand

  if (kind == PYZ_C_BLUR) {   // scipy.ndimage.gaussian_filter, mode "nearest": axis 0, then axis 1, taps -r .. r
    const int r = g.r[s];
    const float *wt = g.bw[s];
    for (int q = tid; q < planes * hw; q += PYZ_CORRUPT_THREADS) {
      const int k = q / hw, p = q - k * hw, y = p / w, xx = p - y * w;
      const float *src = A + k * hw + xx;
      float acc = 0.0f;
      for (int t = -r; t <= r; ++t) acc = fmaf(wt[t < 0 ? -t : t], src[min(max(y + t, 0), h - 1) * w], acc);
      B[q] = acc;
    }
    __syncthreads();
    for (int q = tid; q < planes * hw; q += PYZ_CORRUPT_THREADS) {
      const int k = q / hw, p = q - k * hw, y = p / w, xx = p - y * w;
      const float *src = B + k * hw + y * w;
      float acc = 0.0f;
      for (int t = -r; t <= r; ++t) acc = fmaf(wt[t < 0 ? -t : t], src[min(max(xx + t, 0), w - 1)], acc);
      A[q] = pyz_clip01(acc);
    }
    __syncthreads();
  } else if (kind == PYZ_C_CONTRAST) {   // (v - m) c + m, m the channel's mean: per-thread sums, then a tree over the threads
    for (int k = 0; k < planes; ++k) {
      float acc = 0.0f;
      for (int p = tid; p < hw; p += PYZ_CORRUPT_THREADS) acc += A[k * hw + p];
      red[tid] = acc;
      __syncthreads();
      for (int d = PYZ_CORRUPT_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
      }
      const float m = red[0] / (float)hw;
      __syncthreads();
      for (int p = tid; p < hw; p += PYZ_CORRUPT_THREADS) B[k * hw + p] = pyz_clip01((A[k * hw + p] - m) * c + m);
    }
    __syncthreads();
    res = B;
  } else {   // pixelate: BOX down (horizontal, then vertical), NEAREST up
    const int oh = g.oh[s], ow = g.ow[s];
    int2 *tx = reinterpret_cast<int2 *>(B + planes * hw), *ty = tx + ow;
    for (int q = tid; q < ow + oh; q += PYZ_CORRUPT_THREADS) tx[q] = q < ow ? pyz_box_taps(q, w, ow) : pyz_box_taps(q - ow, h, oh);
    __syncthreads();
    for (int q = tid; q < planes * h * ow; q += PYZ_CORRUPT_THREADS) {   // B (planes, h, ow)
      const int k = q / (h * ow), p = q - k * (h * ow), y = p / ow, ii = p - y * ow;
      const int2 t = tx[ii];
      const float *src = A + k * hw + y * w;
      float acc = 0.0f;
      for (int j = t.x; j < t.y; ++j) acc += src[j];
      B[q] = acc / (float)(t.y - t.x);
    }
    __syncthreads();
    for (int q = tid; q < planes * oh * ow; q += PYZ_CORRUPT_THREADS) {   // A (planes, oh, ow)
      const int k = q / (oh * ow), p = q - k * (oh * ow), yy = p / ow, ii = p - yy * ow;
      const int2 t = ty[yy];
      const float *src = B + k * (h * ow) + ii;
      float acc = 0.0f;
      for (int j = t.x; j < t.y; ++j) acc += src[j * ow];
      A[q] = acc / (float)(t.y - t.x);
    }
    __syncthreads();
    for (int p = tid; p < hw; p += PYZ_CORRUPT_THREADS) {
      const int y = p / w, xx = p - y * w;
      const int sp = pyz_nearest_src(y, h, oh) * ow + pyz_nearest_src(xx, w, ow);
      float v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = pyz_clip01(A[(planes == 3 ? k : 0) * (oh * ow) + sp]);
      pyz_corrupt_emit(g, o, p, v[0], v[1], v[2]);
    }
    return;
  }
  for (int p = tid; p < hw; p += PYZ_CORRUPT_THREADS)
    pyz_corrupt_emit(g, o, p, res[p], res[(planes == 3 ? 1 : 0) * hw + p], res[(planes == 3 ? 2 : 0) * hw + p]);
}

// LDS bytes of the staged kinds: the reduction row, image and scratch copy as three channels, and the tap table of the
// longest axes pixelate can meet.  (A grey image uses a third of the two copies; the limit is one for both channel counts.)
static inline size_t pyz_corrupt_lds(int h, int w) {
  return sizeof(float) * (PYZ_CORRUPT_THREADS + (size_t)2 * 3 * h * w) + sizeof(int2) * ((size_t)h + w);
}

// fills the per-severity tables of g; PYZ_E_INVALID (with the pyz_last_error text set) for a severity outside 1..5
static inline int pyz_corrupt_tables(CorruptArgs &g, const int32_t *severities, int n_sev) {
  for (int s = 0; s < n_sev; ++s) {
    const int sv = severities[s];
    if (sv < 1 || sv > 5) return pyz_fail(PYZ_E_INVALID, "severity %d outside 1..5", sv);
    g.sev[s] = sv;
    const double c = PYZ_CORRUPT_C[g.kind][sv - 1];
    g.c0[s] = (float)c;
    g.c1[s] = g.kind == PYZ_C_SATURATE ? (float)PYZ_SATURATE_C1[sv - 1] : 0.0f;
    if (g.kind == PYZ_C_BLUR) {
      const int r = (int)(4.0 * c + 0.5);
      double wsum = 0.0, wk[PYZ_CORRUPT_MAX_R + 1];
      for (int k = 0; k <= r; ++k) {
        wk[k] = std::exp(-0.5 * (double)(k * k) / (c * c));
        wsum += k ? 2.0 * wk[k] : wk[k];
      }
      g.r[s] = r;
      for (int k = 0; k <= r; ++k) g.bw[s][k] = (float)(wk[k] / wsum);
    }
    if (g.kind == PYZ_C_PIXELATE) {   // Robustness.py:89: int(shape * c)
      g.oh[s] = std::max(1, (int)(g.h * c));
      g.ow[s] = std::max(1, (int)(g.w * c));
    }
  }
  return PYZ_OK;
}

// ---------------------------------------------------------------- scoring
#define PYZ_SCORE_ROWS_PER_BLOCK 2048   // regression: rows per workgroup (8 per thread)

// kind 0, classification: thread = row, grid (cdiv(n, 256), groups); np.argmax (the FIRST maximum) for C >= 2, mean > 0.5
// for C == 1; the wrong rows of a wave go to wrong[group] in one integer atomic.
// kind 1, regression: grid (cdiv(n, PYZ_SCORE_ROWS_PER_BLOCK), groups); workgroup (b, group) sums (mean - y)^2 over its rows
// per column in float64 -> part[(group * C + c) * gridDim.x + b]; k_score_sum adds the workgroups in order.
__global__ void __launch_bounds__(256) k_score_rows(const float *mean, long long n, int C, const void *yv, int kind,
                                                    unsigned long long *wrong, double *part) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const float *m = mean + (long long)blockIdx.y * n * C;
  if (kind == 0) {
    const int32_t *y = static_cast<const int32_t *>(yv);
    const long long row = (long long)blockIdx.x * 256 + tid;
    bool bad = false;
    if (row < n) {
      const float *mr = m + row * C;
      int best = 0;
      if (C == 1) {
        best = mr[0] > 0.5f ? 1 : 0;
      } else {
        float top = mr[0];
        for (int a = 1; a < C; ++a) {
          const float v = mr[a];
          if (v > top) {
            top = v;
            best = a;
          }
        }
      }
      bad = best != y[row];
    }
    const unsigned long long votes = __ballot(bad);
    if ((tid & 63) == 0 && votes) atomicAdd(wrong + blockIdx.y, (unsigned long long)__popcll(votes));
    return;
  }
  const float *y = static_cast<const float *>(yv);
  const long long r0 = (long long)blockIdx.x * PYZ_SCORE_ROWS_PER_BLOCK;
  const long long r1 = min(n, r0 + (long long)PYZ_SCORE_ROWS_PER_BLOCK);
  for (int c = 0; c < C; ++c) {
    double acc = 0.0;
    for (long long r = r0 + tid; r < r1; r += 256) {
      const double d = (double)m[r * C + c] - (double)y[r * C + c];
      acc += d * d;
    }
    red[tid] = acc;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
      if (tid < d) red[tid] += red[tid + d];
      __syncthreads();
    }
    if (tid == 0) part[((long long)blockIdx.y * C + c) * gridDim.x + blockIdx.x] = red[0];
    __syncthreads();
  }
}

// out[j] = the nblk partial sums of j = group * C + c, added in block order
__global__ void __launch_bounds__(256) k_score_sum(const double *part, int nblk, int total, double *out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= total) return;
  double acc = 0.0;
  for (int b = 0; b < nblk; ++b) acc += part[(long long)j * nblk + b];
  out[j] = acc;
}
