// pyz_predict_moments.h -- per-row predictive moments of a Monte-Carlo read-out, in one launch per chunk of draws.
//
// Replaces the draw-by-draw, row-by-row loop of Metrics.classification_uncertainty
// (Pyesian/visualisations/Metrics.py), which needs of the (draws, rows, C) sample tensor only, per row j,
//
//   mean[j][a]  = sum_s p[s][j][a] * (1 / n_samples)        (what pyz_predict's d_mean holds, bit for bit)
//   m2[j][a][b] = sum_s p[s][j][a] * p[s][j][b]             (the full C x C matrix, row-major)
//
// p = k_predict_rows' value: softmax of the last layer's logits where the last activation is softmax, then NaN -> 0.
// The kernel reads the plan's last-layer buffer (S, max_batch, C) once, normalises in LDS and keeps the sums in
// registers: the sample tensor is never written, let alone copied to the host.
//
// Decomposition.  A workgroup of 256 threads owns R = max(1, 256 / C) consecutive rows, whose C logits per draw are ONE
// contiguous run of R * C floats: staged through LDS with coalesced dword loads, PM_AHEAD draws ahead in registers (a
// workgroup's draws form a serial chain; without the run-ahead every draw pays a full memory round trip).  Thread
// (j, a) owns output row a of row j's matrix: PM_TB accumulators over b in [b0, b0 + PM_TB), b0 = PM_TB * blockIdx.y
// (wider C: more workgroups along y, each normalising the rows again), and, in the b0 = 0 workgroups, mean[j][a].
// C > 256: R = 1 and blockIdx.z splits a into runs of 256.  Every output element is one thread's strictly sequential
// float32 sum in draw order, continued across chunks through `accumulate`: no atomics, the same bits however the
// draws are chunked.  fmaf(pa, pb, acc) rounds the same for (a, b) and (b, a): m2 is symmetric bit for bit.
//
// The softmax is k_predict_rows' arithmetic (pyz_kernels.h), spread over the threads of a row: the same max loop, the
// same expf(z - mx) terms summed in the same column order, the same lse = mx + logf(se) and expf(z - lse); the mean is
// k_predict_mean's `acc += p * inv_total` in draw order.
#pragma once

#include <algorithm>

#include "pyz_common.h"

#define PM_TB 16      // accumulators over b per thread (four float4 LDS reads per draw)
#define PM_AHEAD 4    // draws in flight per thread

struct PredictMomentsArgs {
  const float *last;      // (S, max_batch, C) logits / outputs of this chunk of draws
  long long pstride;      // max_batch * C
  int C, CP;              // outputs per row; LDS row stride (C rounded up to 4, the pad columns stay 0)
  int R, CA;              // rows per workgroup; a-columns per workgroup (min(C, 256))
  int softmax;
  int n, S;               // rows; draws of this chunk
  float *mean;            // (n, C)
  float *m2;              // (n, C, C)
  int accumulate;         // an earlier chunk of draws already stands in mean / m2: continue its sums
  float inv_total;        // 1 / n_samples
};

// LDS floats: two buffers of R x CP values (draw s in buffer s & 1), R x CP exp terms, R row maxima
static inline size_t pyz_predict_moments_lds(int R, int CP) { return ((size_t)3 * R * CP + R) * sizeof(float); }

// ONE: C <= 256, every thread stages, normalises and accumulates ONE element (j, a) of the workgroup's R x C block, so
// nothing per draw is a loop or a division (a workgroup's draws are a serial chain with one or two waves per SIMD: the
// instructions of a draw are its time).  !ONE: C > 256, R = 1, a thread stages and normalises every 256th column.
template <bool ONE>
__device__ __forceinline__ void pyz_predict_moments_body(const PredictMomentsArgs &g, float *pm_lds) {
  const int C = g.C, CP = g.CP, R = g.R, S = g.S, softmax = g.softmax;
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * R;
  const int rows = (int)min((long long)R, (long long)g.n - row0);   // >= 1: the grid is cdiv(n, R)
  const int RC = rows * C;                                           // this workgroup's values per draw
  const int b0 = blockIdx.y * PM_TB;
  float *es = pm_lds + 2 * R * CP, *mxs = es + R * CP;
  for (int i = tid; i < 2 * R * CP; i += 256) pm_lds[i] = 0.0f;      // (the pad columns: never written again)
  __syncthreads();

  const int j = tid / g.CA, a = blockIdx.z * g.CA + tid % g.CA;
  const bool own = j < rows && a < C;                                // (ONE: the same as tid < RC, and tid = j * C + a)
  const int zrow = j * CP, zoff = zrow + a;
  const bool first_tile = blockIdx.y == 0;
  float acc[PM_TB], macc = 0.0f;
#pragma unroll
  for (int i = 0; i < PM_TB; ++i) acc[i] = 0.0f;
  const long long orow = own ? (row0 + j) * C + a : 0;               // element of mean, row of m2
  if (own && g.accumulate) {
    if (first_tile) macc = g.mean[orow];
#pragma unroll
    for (int i = 0; i < PM_TB; ++i)
      if (b0 + i < C) acc[i] = g.m2[orow * C + b0 + i];
  }

  const float *src = g.last + row0 * C;
  // this thread's first staged value runs ahead.  The loads are UNCONDITIONAL (a thread past the block reads its
  // element 0, a draw past the chunk is the last draw again): a load under a branch is waited for at the branch's
  // join, i.e. at once, and every draw would pay the round trip the run-ahead is there to hide
  const float *mine = src + (tid < RC ? tid : 0);
  float zr[PM_AHEAD];
#pragma unroll
  for (int u = 0; u < PM_AHEAD; ++u) zr[u] = mine[min(u, S - 1) * g.pstride];

  for (int s0 = 0; s0 < S; s0 += PM_AHEAD) {
#pragma unroll
    for (int u = 0; u < PM_AHEAD; ++u) {
      const int s = s0 + u;
      float zc = zr[u];
      zr[u] = mine[min(s + PM_AHEAD, S - 1) * g.pstride];            // (outside the branch below, for the same reason)
      if (s < S) {                                                   // (uniform)
        float *zs = pm_lds + (u & 1) * R * CP;                       // PM_AHEAD is even: s & 1 == u & 1
        if (!softmax) zc = (zc != zc) ? 0.0f : zc;
        if (ONE) {
          if (own) zs[zoff] = zc;
        } else {
          const float *ds = src + s * g.pstride;
          for (int e = tid; e < RC; e += 256) {
            float v = e == tid ? zc : ds[e];
            if (!softmax) v = (v != v) ? 0.0f : v;
            zs[(e / C) * CP + e % C] = v;
          }
        }
        __syncthreads();
        if (softmax) {
          float mx = 0.0f;
          if (ONE) {
            if (own) {
              const float *z = zs + zrow;
              mx = z[0];
              for (int k = 1; k < C; ++k) mx = fmaxf(mx, z[k]);
              es[zoff] = expf(zc - mx);
            }
          } else {
            for (int e = tid; e < RC; e += 256) {
              const int jj = e / C, c = e % C;
              const float *z = zs + jj * CP;
              mx = z[0];
              for (int k = 1; k < C; ++k) mx = fmaxf(mx, z[k]);
              es[jj * CP + c] = expf(z[c] - mx);
              if (c == 0) mxs[jj] = mx;
            }
          }
          __syncthreads();
          if (ONE) {
            if (own) {
              const float *t = es + zrow;
              float se = 0.0f;
              for (int k = 0; k < C; ++k) se += t[k];
              const float lse = mx + logf(se);
              float v = expf(zc - lse);
              zs[zoff] = (v != v) ? 0.0f : v;
            }
          } else {
            for (int e = tid; e < RC; e += 256) {
              const int jj = e / C, c = e % C;
              const float *t = es + jj * CP;
              float se = 0.0f;
              for (int k = 0; k < C; ++k) se += t[k];
              const float lse = mxs[jj] + logf(se);
              float v = expf(zs[jj * CP + c] - lse);
              zs[jj * CP + c] = (v != v) ? 0.0f : v;
            }
          }
          __syncthreads();
        }
        if (own) {
          const float *p = zs + zrow;
          const float pa = p[a];
          if (first_tile) macc += pa * g.inv_total;
#pragma unroll
          for (int q = 0; q < PM_TB / 4; ++q)
            if (b0 + 4 * q < CP) {
              const float4 pb = *reinterpret_cast<const float4 *>(p + b0 + 4 * q);
              acc[4 * q + 0] = fmaf(pa, pb.x, acc[4 * q + 0]);
              acc[4 * q + 1] = fmaf(pa, pb.y, acc[4 * q + 1]);
              acc[4 * q + 2] = fmaf(pa, pb.z, acc[4 * q + 2]);
              acc[4 * q + 3] = fmaf(pa, pb.w, acc[4 * q + 3]);
            }
        }
      }
    }
  }
  if (own) {
    if (first_tile) g.mean[orow] = macc;
#pragma unroll
    for (int i = 0; i < PM_TB; ++i)
      if (b0 + i < C) g.m2[orow * C + b0 + i] = acc[i];
  }
}

__global__ void __launch_bounds__(256) k_predict_moments(PredictMomentsArgs g) {
  extern __shared__ __attribute__((aligned(16))) float pm_lds[];
  if (g.C <= 256) pyz_predict_moments_body<true>(g, pm_lds);
  else pyz_predict_moments_body<false>(g, pm_lds);
}

// false: a row of C values does not fit the LDS of a compute unit (C beyond ~13 000, where ONE row's C x C matrix
// would itself take 0.7 GB)
static inline bool pyz_launch_predict_moments(PredictMomentsArgs g, hipStream_t st) {
  g.CP = (g.C + 3) & ~3;
  g.CA = std::min(g.C, 256);
  g.R = std::max(1, 256 / g.C);
  const size_t lds = pyz_predict_moments_lds(g.R, g.CP);
  if (lds > 160 * 1024) return false;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(k_predict_moments), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return false;
  PYZ_LAUNCH(k_predict_moments, dim3((unsigned)((g.n + g.R - 1) / g.R), (unsigned)((g.C + PM_TB - 1) / PM_TB),
                                     (unsigned)((g.C + g.CA - 1) / g.CA)),
             dim3(256), lds, st, g);
  return true;
}
