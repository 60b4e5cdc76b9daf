// pyz_conv.h -- the convolutional front end ("stem") in front of the Dense stack: Conv2D and MaxPooling2D, NHWC, float32.
//
// Replaces Keras Conv2D / MaxPooling2D forward and their part of tf.GradientTape.gradient for the models the reference's
// builder emits (Pyesian utils.py:129-150) and its image script trains (tests/tf_dataset_test.py:42-57).
//
// Design (gfx950), after the tile design at the head of pyz_gemm.h:
//   * a convolution is an implicit GEMM: rows = the M = batch * OH * OW output positions, reduction = the K = kh * kw * cin
//     taps plus the bias row, columns = cout.  A conv kernel (kh, kw, cin, cout) read as a (K, cout) matrix followed by its
//     bias IS the augmented [W; b] of pyz_gemm.h, so the flat layout needs no repacking;
//   * one wave computes a 32 x 32 tile with v_mfma_f32_32x32x2_f32; the S waves of a workgroup take interleaved steps of
//     the reduction and combine through LDS in a fixed order (pyz_tile_epilogue);
//   * the A operand is gathered in the load: tap k = (i, j, c) of row (b, oy, ox) is x[b, oy + i - pt, ox + j - pl, c], zero
//     outside the image.  The decomposition of k is a table made once per layer on the host ({i, j}, offset) that the
//     workgroup copies to LDS: a step costs one LDS read, two compares and two loads -- no integer division;
//   * the weight gradient [dW; db] = A^T delta reduces over M, which is long (33 792 rows for 33 images of 32 x 32): it is
//     cut into G ranges of rows, one workgroup each, whose raw 32 x 32 partial tiles go to a slab that k_conv_wgrad_reduce
//     adds in range order.  No atomics anywhere: a repeated call gives the same bits;
//   * the data gradient and the two pooling kernels are gathers: every output element is owned by one thread;
//   * blockIdx.y is the particle, as everywhere in this library.
#pragma once

#include "pyz_gemm.h"

#define PYZ_STEM_CONV 0
#define PYZ_STEM_POOL 1
#define PYZ_STEM_MAX_OPS 16
#define PYZ_CONV_MAX_K 4094      // taps of one filter: the tap table (8 bytes a tap, + bias + padding) stays within 32 KiB of LDS
#define PYZ_CONV_MAX_ROWS (1 << 24)   // rows of one launch: pyz_fdiv converts a row number to float exactly
#define PYZ_CONV_WAVES 4         // at most this many waves split a tile's reduction

// tap table entry: x = (i << 16) | j for a tap, PYZ_TAP_BIAS for the bias row, PYZ_TAP_NONE past it; y = (i * W + j) * C + c
#define PYZ_TAP_BIAS (-1)
#define PYZ_TAP_NONE (-2)

// n / d for 0 <= n < 2^24 through a float reciprocal: the product is within one of the quotient, the loops settle it
__device__ __forceinline__ int pyz_fdiv(const int n, const int d, const float inv, int &rem) {
  int q = (int)((float)n * inv);
  int r = n - q * d;
  while (r < 0) {
    --q;
    r += d;
  }
  while (r >= d) {
    ++q;
    r -= d;
  }
  rem = r;
  return q;
}

struct ConvArgs {
  const float *in;            // (P or 1, images, H, W, C)
  long long in_pstride;       // 0 for the data batch
  const float *theta;         // (P, D_total)
  long long theta_pstride;
  long long w_off;            // this layer's kernel in the flat vector (bias follows)
  float *out;                 // forward: (P, max_batch, OH, OW, N)
  long long out_pstride;
  const int32_t *row_idx;     // first layer only: image of batch row b
  const int2 *ktab;           // KT tap entries
  int M;                      // batch * OH * OW
  int H, W, C, OH, OW, N, K, KT, pt, pl, act;
  float inv_ohw, inv_ow;
  // weight gradient
  const float *delta;         // (P, max_batch, OH, OW, N)
  long long delta_pstride;
  float *part;                // (P, G, tiles, 1024) raw partial tiles
  int G, rows_per_g;
  float *grad;                // (P, D_total)
  long long grad_pstride;
  // data gradient
  const float *below;         // output of the conv that produced `in` (for act'), or null
  long long below_pstride;
  int act_below, kh, kw, batch;
};

// ---------------------------------------------------------------- forward
__global__ void __launch_bounds__(64 * PYZ_CONV_WAVES) k_conv_fwd(ConvArgs g) {
  extern __shared__ float lds[];
  int2 *tab = reinterpret_cast<int2 *>(lds);
  float *red = lds + 2 * g.KT;
  const int S = blockDim.x >> 6, w = pyz_wave_id(), l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  for (int e = threadIdx.x; e < g.KT; e += blockDim.x) tab[e] = g.ktab[e];
  __syncthreads();
  const int tiles_n = (g.N + 31) >> 5;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n, p = blockIdx.y;
  const int M = g.M, N = g.N, H = g.H, W = g.W;
  const int m = tm * 32 + r, n = tn * 32 + r;
  const bool row_ok = m < M, col_ok = n < N;
  int iy0 = 0, ix0 = 0;
  long long boff = 0;
  if (row_ok) {
    int pos, ox;
    const int b = pyz_fdiv(m, g.OH * g.OW, g.inv_ohw, pos);
    const int oy = pyz_fdiv(pos, g.OW, g.inv_ow, ox);
    const long long img = g.row_idx ? (long long)g.row_idx[b] : (long long)b;
    iy0 = oy - g.pt;
    ix0 = ox - g.pl;
    boff = (img * H + iy0) * (long long)W * g.C + (long long)ix0 * g.C;
  }
  const float *xp = g.in + p * g.in_pstride;
  const float *wl = g.theta + p * g.theta_pstride + g.w_off;
  f32x16 acc = {0};
  const int steps = g.KT >> 1;
  pyz_steps1_all(
      0, (steps - w + S - 1) / S, acc,
      [&](int u, float &a, float &b) {
        const int k = 2 * (w + S * u) + h;
        const int2 t = tab[k];
        a = 0.0f;
        if (t.x >= 0) {
          const bool ok = row_ok && (unsigned)(iy0 + (t.x >> 16)) < (unsigned)H && (unsigned)(ix0 + (t.x & 0xffff)) < (unsigned)W;
          if (ok) a = xp[boff + t.y];
        } else if (t.x == PYZ_TAP_BIAS) {
          a = 1.0f;
        }
        b = (t.x != PYZ_TAP_NONE && col_ok) ? wl[(long long)k * N + n] : 0.0f;
      },
      PyzNoFix());
  float *op = g.out + p * g.out_pstride;
  const int act = g.act;
  pyz_tile_epilogue(acc, red, [&](int ro, int co, float v) {
    const int mm = tm * 32 + ro, nn = tn * 32 + co;
    if (mm < M && nn < N) op[(long long)mm * N + nn] = pyz_act(v, act);
  });
}

// ---------------------------------------------------------------- weight gradient
// part[p][range][tile] = A^T delta over the range's rows; tile (tk, tn) holds taps 32 tk .. and columns 32 tn ..
// The range is walked in chunks of PYZ_WGRAD_CHUNK rows.  Where a row sits -- its image through row_idx, its (oy, ox) -- is
// worked out once per chunk, by all threads, into LDS ({offset of the window's corner in x}, {oy - pt, ox - pl}); a
// reduction step then costs one LDS read, two compares and two loads, like the forward's: no division and no row_idx load
// stands between a step's loads.  The waves add their steps chunk after chunk into one accumulator each: a fixed order.
#define PYZ_WGRAD_CHUNK 512
__global__ void __launch_bounds__(64 * PYZ_CONV_WAVES) k_conv_wgrad(ConvArgs g) {
  extern __shared__ float red[];
  const int S = blockDim.x >> 6, w = pyz_wave_id(), l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  long long *corner = reinterpret_cast<long long *>(red + (S > 1 ? S * 1024 : 0));   // (S * 4096 bytes: 8-byte aligned)
  int2 *yx = reinterpret_cast<int2 *>(corner + PYZ_WGRAD_CHUNK);
  const int tiles_n = (g.N + 31) >> 5, tiles = ((g.K + 1 + 31) >> 5) * tiles_n;
  const int rg = blockIdx.x / tiles, tile = blockIdx.x - rg * tiles, p = blockIdx.y;
  const int tk = tile / tiles_n, tn = tile - tk * tiles_n;
  const int M = g.M, N = g.N, H = g.H, W = g.W, C = g.C, OHW = g.OH * g.OW;
  const int k = tk * 32 + r, n = tn * 32 + r;
  const int2 t = k < g.KT ? g.ktab[k] : make_int2(PYZ_TAP_NONE, 0);
  const bool col_ok = n < N;
  const int ti = t.x >> 16, tj = t.x & 0xffff;
  const int m0 = rg * g.rows_per_g, m1 = min(M, m0 + g.rows_per_g);
  const float *xp = g.in + p * g.in_pstride;
  const float *dp = g.delta + p * g.delta_pstride;
  f32x16 acc = {0};
  for (int c0 = m0; c0 < m1; c0 += PYZ_WGRAD_CHUNK) {   // (uniform)
    const int rows = min(PYZ_WGRAD_CHUNK, m1 - c0);
    if (c0 > m0) __syncthreads();   // every wave is done with the last chunk's table
    for (int e = threadIdx.x; e < rows; e += blockDim.x) {
      int pos, ox;
      const int bi = pyz_fdiv(c0 + e, OHW, g.inv_ohw, pos);
      const int oy = pyz_fdiv(pos, g.OW, g.inv_ow, ox);
      const long long img = g.row_idx ? (long long)g.row_idx[bi] : (long long)bi;
      corner[e] = (img * H + (oy - g.pt)) * (long long)W * C + (long long)(ox - g.pl) * C;
      yx[e] = make_int2(oy - g.pt, ox - g.pl);
    }
    __syncthreads();
    const int steps = (rows + 1) >> 1;
    pyz_steps1_all(
        0, (steps - w + S - 1) / S, acc,
        [&](int u, float &a, float &b) {
          const int e = 2 * (w + S * u) + h;
          a = 0.0f;
          b = 0.0f;
          if (e < rows) {
            if (t.x >= 0) {
              const int2 q = yx[e];
              if ((unsigned)(q.x + ti) < (unsigned)H && (unsigned)(q.y + tj) < (unsigned)W) a = xp[corner[e] + t.y];
            } else if (t.x == PYZ_TAP_BIAS) {
              a = 1.0f;
            }
            if (col_ok) b = dp[(long long)(c0 + e) * N + n];
          }
        },
        PyzNoFix());
  }
  float *op = g.part + (((long long)p * g.G + rg) * tiles + tile) * 1024;
  pyz_tile_epilogue(acc, red, [&](int ro, int co, float v) { op[ro * 32 + co] = v; });
}

// grad[p][w_off + k N + n] = the G partial sums of (k, n), added in a fixed order: a workgroup owns 16 elements; slice q of
// its 16 adds the ranges q, q + 16, ... of each in turn (256 threads, so that hundreds of partials per element are
// not one thread's serial chain of loads), then one thread per element adds the 16 slice sums in slice order
__global__ void __launch_bounds__(256) k_conv_wgrad_reduce(ConvArgs g) {
  __shared__ float sl[16][17];
  const int el = threadIdx.x & 15, q = threadIdx.x >> 4, p = blockIdx.y;
  const int N = g.N, E = (g.K + 1) * N;
  const int e = blockIdx.x * 16 + el;
  float s = 0.0f;
  if (e < E) {
    const int k = e / N, n = e - k * N;
    const int tiles_n = (N + 31) >> 5, tiles = ((g.K + 1 + 31) >> 5) * tiles_n;
    const int tile = (k >> 5) * tiles_n + (n >> 5), idx = (k & 31) * 32 + (n & 31);
    const float *pp = g.part + ((long long)p * g.G * tiles + tile) * 1024 + idx;
    for (int rg = q; rg < g.G; rg += 16) s += pp[(long long)rg * tiles * 1024];
  }
  sl[q][el] = s;
  __syncthreads();
  if (q == 0 && e < E) {
    float t = sl[0][el];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += sl[i][el];
    g.grad[p * g.grad_pstride + g.w_off + e] = t;
  }
}

// ---------------------------------------------------------------- data gradient (gather form)
// out[b, y, x, c] = ( sum_{i, j, n} delta[b, y - i + pt, x - j + pl, n] W[i, j, c, n] ) * act'(below[b, y, x, c])
__global__ void k_conv_dgrad(ConvArgs g) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  const int H = g.H, W = g.W, C = g.C, N = g.N;
  if (e >= (long long)g.batch * H * W * C) return;
  const int c = (int)(e % C);
  const long long q = e / C;
  const int x = (int)(q % W), y = (int)((q / W) % H), b = (int)(q / ((long long)W * H));
  const float *dp = g.delta + p * g.delta_pstride;
  const float *wl = g.theta + p * g.theta_pstride + g.w_off;
  float s = 0.0f;
  for (int i = 0; i < g.kh; ++i) {
    const int oy = y - i + g.pt;
    if ((unsigned)oy >= (unsigned)g.OH) continue;
    for (int j = 0; j < g.kw; ++j) {
      const int ox = x - j + g.pl;
      if ((unsigned)ox >= (unsigned)g.OW) continue;
      const float *d = dp + (((long long)b * g.OH + oy) * g.OW + ox) * N;
      const float *wr = wl + ((long long)(i * g.kw + j) * C + c) * N;
      for (int n = 0; n < N; ++n) s = fmaf(d[n], wr[n], s);
    }
  }
  if (g.below) s *= pyz_act_grad(g.below[p * g.below_pstride + e], g.act_below);
  g.out[p * g.out_pstride + e] = s;
}

// ---------------------------------------------------------------- max pooling
struct PoolArgs {
  const float *in;            // (P, max_batch, H, W, C): the conv output beneath
  long long in_pstride;
  float *out;                 // (P, max_batch, OH, OW, C)
  long long out_pstride;
  int32_t *win;               // forward: the winner's y * W + x, shaped like out
  const float *dout;          // backward: d loss / d out
  float *din;                 // backward: d loss / d (pre-activation of the conv beneath), shaped like in
  int batch, H, W, C, OH, OW, ph, pw, act_below;
};

// the first maximum in row-then-column scan order; a NaN wins and stays (it propagates, like tf.nn.max_pool)
__global__ void k_pool_fwd(PoolArgs g) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  const int C = g.C, OW = g.OW, OH = g.OH;
  if (e >= (long long)g.batch * OH * OW * C) return;
  const int c = (int)(e % C);
  const long long q = e / C;
  const int ox = (int)(q % OW), oy = (int)((q / OW) % OH), b = (int)(q / ((long long)OW * OH));
  const float *ip = g.in + p * g.in_pstride + (long long)b * g.H * g.W * C + c;
  const int y0 = oy * g.ph, x0 = ox * g.pw;
  float best = ip[((long long)y0 * g.W + x0) * C];
  int at = y0 * g.W + x0;
  for (int i = 0; i < g.ph; ++i)
    for (int j = 0; j < g.pw; ++j) {
      const int pos = (y0 + i) * g.W + x0 + j;
      const float v = ip[(long long)pos * C];
      if (v > best || (v != v && best == best)) {
        best = v;
        at = pos;
      }
    }
  g.out[p * g.out_pstride + e] = best;
  g.win[p * g.out_pstride + e] = at;
}

// din[b, y, x, c] = (the window's winner is (y, x) ? dout[window] : 0) * act'(in[b, y, x, c]); rows and columns of the
// remainder belong to no window
__global__ void k_pool_bwd(PoolArgs g) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  const int C = g.C, W = g.W, H = g.H;
  if (e >= (long long)g.batch * H * W * C) return;
  const int c = (int)(e % C);
  const long long q = e / C;
  const int x = (int)(q % W), y = (int)((q / W) % H), b = (int)(q / ((long long)W * H));
  const int oy = y / g.ph, ox = x / g.pw;
  float d = 0.0f;
  if (oy < g.OH && ox < g.OW) {
    const long long o = p * g.out_pstride + (((long long)b * g.OH + oy) * g.OW + ox) * C + c;
    if (g.win[o] == y * W + x) d = g.dout[o] * pyz_act_grad(g.in[p * g.in_pstride + e], g.act_below);
  }
  g.din[p * g.in_pstride + e] = d;
}

// (P, batch, F) caller rows <-> the stem's (P, max_batch, F) buffers; SEED: times act'(features) on the way in
template <bool SEED>
__global__ void k_stem_rows(const float *src, long long src_pstride, float *dst, long long dst_pstride, long long n,
                            const float *feat, long long feat_pstride, int act) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (e >= n) return;
  float v = src[p * src_pstride + e];
  if (SEED) v *= pyz_act_grad(feat[p * feat_pstride + e], act);
  dst[p * dst_pstride + e] = v;
}
