// pyz_surface.h -- what a decision-surface plot needs of a Monte-Carlo read-out, made and kept on the device.
//
// Plotter.plot_decision_boundaries / plot_uncertainty_area (Pyesian/visualisations/Plotter.py:54-78,100-135) read the
// posterior out on a dense n1 x n2 grid (10^6 rows at granularity 1e-3) and use of the (draws, rows, C) sample tensor only
// one column per draw (the contour lines) and, per row, three numbers of the mean (its maximum, where it is, its entropy).
//
//   k_grid_rows        rows [row0, row0 + n) of the grid, mapped back to input space: row r has i = r / n2, j = r % n2
//                      (tf.meshgrid(indexing='ij') + reshape(-1), :132-133), u = a0 + (float)i * da, v = b0 + (float)j * db,
//                      out[r - row0][k] = u * B[k][0] + v * B[k][1] (grid @ base_matrix^T, :134).  Every product and sum
//                      is rounded to float32 on its own, so a NumPy float32 restatement gives the same bits: the
//                      function is compiled with `fp contract(off)` (HIP's __fmul_rn / __fadd_rn are plain `x * y` /
//                      `x + y` in this toolchain's headers and contract to an fma once inlined: measured, one ulp off).
//                      One thread per output element, coalesced stores.
//   k_predict_surface  one launch per chunk of draws, in place of k_predict_rows + k_predict_mean:
//                        cols[s][j] = p[s][j][column]                       (optional)
//                        mean[j][a] = sum_s p[s][j][a] * (1 / n_samples)    (pyz_predict's d_mean, bit for bit)
//                      and, in the launch of the last chunk, of the finished mean row q (C == 1: the pair (1 - m, m),
//                      Plotter.py:37-39,49-51,68-70):
//                        top[j] = max_a q_a, cls[j] = the first index of the maximum (np.argmax),
//                        ent[j] = -sum_a q_a * logf(q_a + 1e-5f), a sequential float32 sum in column order (:366).
//                      p = k_predict_rows' value (pyz_kernels.h): softmax where the last activation is softmax, NaN -> 0.
//
// Decomposition of k_predict_surface, after k_predict_moments (pyz_predict_moments.h): a workgroup of 256 threads owns
// R = max(1, 256 / C) consecutive rows, whose C logits per draw are ONE contiguous run of R * C floats; thread tid stages
// element tid of the run, PS_AHEAD draws ahead in registers, with unconditional loads.  The softmax is k_predict_rows'
// arithmetic: the same max loop, the same expf(z - mx) terms summed in column order, the same lse = mx + logf(se) and
// expf(z - lse).  Nobody reads another thread's p here, so one LDS buffer and two barriers per draw do (a linear last
// layer needs neither).  The mean is k_predict_mean's `acc += p * inv_total` in draw order, continued across chunks
// through `accumulate`; the thread that owns (row, column) also stores the draw's column value.  In the last chunk the
// finished mean row goes back through LDS and one thread per row runs plain sequential loops: no atomics, no cross-lane
// reduction whose order could vary, the same bits however the draws are chunked.  C > 256: one row per workgroup, a
// thread owns every 256th column and the row's mean is accumulated in LDS (one owner per element, still in draw order).
#pragma once

#include <algorithm>

#include "pyz_common.h"

#define PS_AHEAD 4    // draws in flight per thread

__global__ void k_grid_rows(const float *__restrict__ basis, int d, float a0, float da, float b0, float db, int n2,
                            long long row0, long long n_out, float *__restrict__ out) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_out) return;
  const long long r = row0 + e / d;
  const int k = (int)(e % d);
  const float u = a0 + (float)(r / n2) * da;
  const float v = b0 + (float)(r % n2) * db;
  out[e] = u * basis[2 * k] + v * basis[2 * k + 1];
}

struct PredictSurfaceArgs {
  const float *last;      // (S, max_batch, C) logits / outputs of this chunk of draws
  long long pstride;      // max_batch * C
  int C, CP;              // outputs per row; LDS row stride (odd: rows of a wave fall into different banks)
  int R;                  // rows per workgroup
  int softmax;
  int n, S;               // rows; draws of this chunk
  int column;
  float *cols;            // (S, n) of this chunk, or null
  float *mean;            // (n, C)
  int accumulate;         // an earlier chunk of draws already stands in mean: continue its sums
  int finish;             // the last chunk: the mean is complete, write top / cls / ent
  float inv_total;        // 1 / n_samples
  float *top;             // float[n], int32[n], float[n]: each or null
  int *cls;
  float *ent;
};

// LDS floats: R x CP staged values, R x CP exp terms, R x CP means
static inline size_t pyz_predict_surface_lds(int R, int CP) { return (size_t)3 * R * CP * sizeof(float); }

// top / cls / ent of one finished mean row q[0 .. C) (LDS); C == 1: of the pair (1 - m, m)
__device__ __forceinline__ void pyz_surface_summary(const PredictSurfaceArgs &g, const float *q, long long row) {
#pragma clang fp contract(off)
  const float c = 1e-5f;
  float best, acc;
  int at = 0;
  if (g.C == 1) {
    const float m = q[0], q0 = 1.0f - m;
    best = q0;
    if (m > best) {
      best = m;
      at = 1;
    }
    acc = q0 * logf(q0 + c);
    acc = acc + m * logf(m + c);
  } else {
    best = q[0];
    acc = q[0] * logf(q[0] + c);
    for (int k = 1; k < g.C; ++k) {
      const float v = q[k];
      if (v > best) {
        best = v;
        at = k;
      }
      acc = acc + v * logf(v + c);
    }
  }
  if (g.top) g.top[row] = best;
  if (g.cls) g.cls[row] = at;
  if (g.ent) g.ent[row] = -acc;
}

// ONE: C <= 256, every thread stages, normalises and accumulates ONE element (j, a) of the workgroup's R x C block.
// !ONE: C > 256, R = 1, a thread owns every 256th column of the row.
template <bool ONE>
__device__ __forceinline__ void pyz_predict_surface_body(const PredictSurfaceArgs &g, float *zs) {
  const int C = g.C, CP = g.CP, R = g.R, S = g.S, softmax = g.softmax;
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * R;
  const int rows = (int)min((long long)R, (long long)g.n - row0);   // >= 1: the grid is cdiv(n, R)
  const int RC = rows * C;                                           // this workgroup's values per draw
  float *es = zs + R * CP, *ms = es + R * CP;

  const int j = ONE ? tid / C : 0, a = ONE ? tid % C : tid;
  const bool own = tid < RC;                                         // (ONE: tid = j * C + a)
  const int zrow = j * CP, zoff = zrow + a;
  const long long orow = own ? (row0 + j) * C + a : 0;               // ONE: this thread's element of mean
  float macc = 0.0f;
  if (ONE) {
    if (own && g.accumulate) macc = g.mean[orow];
  } else {
    for (int e = tid; e < C; e += 256) ms[e] = g.accumulate ? g.mean[row0 * C + e] : 0.0f;   // (owner-only from here on)
  }
  const bool col_owner = g.cols != nullptr && own && a == g.column;  // (ONE)

  const float *src = g.last + row0 * C;
  // this thread's first staged value runs ahead.  The loads are UNCONDITIONAL (a thread past the block reads its
  // element 0, a draw past the chunk is the last draw again): a load under a branch is waited for at the branch's join
  const float *mine = src + (own ? tid : 0);
  float zr[PS_AHEAD];
#pragma unroll
  for (int u = 0; u < PS_AHEAD; ++u) zr[u] = mine[min(u, S - 1) * g.pstride];

  for (int s0 = 0; s0 < S; s0 += PS_AHEAD) {
#pragma unroll
    for (int u = 0; u < PS_AHEAD; ++u) {
      const int s = s0 + u;
      const float zc = zr[u];
      zr[u] = mine[min(s + PS_AHEAD, S - 1) * g.pstride];            // (outside the branch below, for the same reason)
      if (s < S) {                                                   // (uniform)
        float *colrow = g.cols ? g.cols + (long long)s * g.n + row0 : nullptr;
        if (ONE) {
          float p = zc;
          if (softmax) {
            if (own) zs[zoff] = zc;
            __syncthreads();
            float mx = 0.0f;
            if (own) {
              const float *z = zs + zrow;
              mx = z[0];
              for (int k = 1; k < C; ++k) mx = fmaxf(mx, z[k]);
              es[zoff] = expf(zc - mx);
            }
            __syncthreads();
            if (own) {
              const float *t = es + zrow;
              float se = 0.0f;
              for (int k = 0; k < C; ++k) se += t[k];
              const float lse = mx + logf(se);
              p = expf(zc - lse);
            }
          }
          p = (p != p) ? 0.0f : p;
          if (own) macc += p * g.inv_total;
          if (col_owner) colrow[j] = p;
        } else {
          const float *ds = src + s * g.pstride;
          float mx = 0.0f, lse = 0.0f;
          if (softmax) {
            for (int e = tid; e < C; e += 256) zs[e] = e == tid ? zc : ds[e];
            __syncthreads();
            mx = zs[0];
            for (int k = 1; k < C; ++k) mx = fmaxf(mx, zs[k]);
            for (int e = tid; e < C; e += 256) es[e] = expf(zs[e] - mx);
            __syncthreads();
            float se = 0.0f;
            for (int k = 0; k < C; ++k) se += es[k];
            lse = mx + logf(se);
          }
          for (int e = tid; e < C; e += 256) {
            float p = softmax ? expf(zs[e] - lse) : (e == tid ? zc : ds[e]);
            p = (p != p) ? 0.0f : p;
            ms[e] += p * g.inv_total;
            if (colrow && e == g.column) colrow[0] = p;
          }
        }
      }
    }
  }

  if (ONE) {
    if (own) g.mean[orow] = macc;
  } else {
    for (int e = tid; e < C; e += 256) g.mean[row0 * C + e] = ms[e];
  }
  if (!g.finish) return;                                             // (uniform)
  if (ONE && own) ms[zoff] = macc;
  __syncthreads();
  if (tid < rows) pyz_surface_summary(g, ms + tid * CP, row0 + tid);
}

__global__ void __launch_bounds__(256) k_predict_surface(PredictSurfaceArgs g) {
  extern __shared__ __attribute__((aligned(16))) float ps_lds[];
  if (g.C <= 256) pyz_predict_surface_body<true>(g, ps_lds);
  else pyz_predict_surface_body<false>(g, ps_lds);
}

// does a row of C values fit the LDS of a compute unit (C up to ~13 600)
static inline bool pyz_predict_surface_fits(int C) {
  return pyz_predict_surface_lds(std::max(1, 256 / C), C | 1) <= 160 * 1024;
}

static inline bool pyz_launch_predict_surface(PredictSurfaceArgs g, hipStream_t st) {
  g.CP = g.C | 1;
  g.R = std::max(1, 256 / g.C);
  const size_t lds = pyz_predict_surface_lds(g.R, g.CP);
  if (lds > 160 * 1024) return false;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(k_predict_surface), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return false;
  PYZ_LAUNCH(k_predict_surface, dim3((unsigned)((g.n + g.R - 1) / g.R)), dim3(256), lds, st, g);
  return true;
}
