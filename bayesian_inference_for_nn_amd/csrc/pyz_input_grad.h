// pyz_input_grad.h -- the gradient of the loss with respect to the INPUTS, summed over weight draws.
//
// Replaces tape.gradient(loss, x) summed over nb_samples sampled models and the FGSM step behind it
// (Pyesian/visualisations/Robustness.py:115-144).
//
//   G[m][j] = scale * sum_p sum_n delta0[p][m][n] * W0[p][j][n],   m < rows, j < K = dims[0], n < N = dims[1]
//
// delta0 = d loss / d pre-activation of layer 0 (the plan's delta[0], left there by the head kernel or the data-gradient
// kernels), W0[p] = layer 0's kernel inside draw p's flat vector (the bias row takes no part).  One GEMM whose reduction
// runs over (draw, hidden unit) JOINTLY: the per-draw gradients -- (draws, rows, K) floats, 1.9 GB at 100 draws x 6 000
// rows x 784 -- never exist.  Decomposition of k_dense_bwd_data (pyz_gemm.h): one wave per 32 x 32 output tile, S waves
// of a workgroup split the joint reduction into contiguous ranges (wave w owns draws/units [T w / S, T (w + 1) / S) of the
// draw-major order) and combine through LDS in wave order (pyz_tile_epilogue): no atomics, the same bits on every call.
// The draw index is the OUTER loop of a wave's range, not blockIdx.y: a grid over draws would need either atomics or a
// (draws, rows, K) slab to sum afterwards.
#pragma once

#include <algorithm>

#include "pyz_gemm.h"

struct InputGradArgs {
  const float *delta;         // (P, max_batch, N): delta of layer 0's output
  long long delta_pstride;
  const float *theta;         // (P, D) flat parameters of this chunk of draws
  long long theta_pstride;
  long long w_off;            // offset of layer 0's kernel in the flat vector
  int K, N;                   // input width (output columns of G) / layer 0's width (reduction, with the draws)
  int P;                      // draws of this chunk
  int rows;                   // rows of x
  int vec;                    // float4 loads legal along n
  float scale;
  float *out;                 // (rows, K): G
  int accumulate;             // an earlier chunk of draws already stands in `out`: add to it
  const float *x;             // FGSM (last chunk only, xadv != nullptr): xadv = x + eps * sign(G)
  float *xadv;
  float eps;
};

__global__ void k_input_grad(InputGradArgs g) {
  extern __shared__ float red[];
  const int S = blockDim.x >> 6, w = pyz_wave_id(), l = threadIdx.x & 63;
  const int r = l & 31, h = l >> 5;
  const int rows = g.rows, K = g.K, N = g.N;
  const int tiles_j = (K + 31) >> 5;
  const int tile = pyz_xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (tile / tiles_j) * 32, j0 = (tile % tiles_j) * 32;
  if (m0 >= rows) return;
  const int m = min(m0 + r, rows - 1), j = min(j0 + r, K - 1);
  const float *ap = g.delta + (long long)m * N;
  const float *wp = g.theta + g.w_off + (long long)j * N;
  f32x16 acc = {0};
  const int c8 = g.vec ? (N >> 3) : 0;
  if (c8 > 0) {   // float4 steps: this wave's range of the P * c8 chunks, draw by draw
    const int T = g.P * c8;
    int c = (int)(((long long)T * w) / S);
    const int ce = (int)(((long long)T * (w + 1)) / S);
    while (c < ce) {
      const int p = c / c8, c0 = c - p * c8, c1 = min(c8, c0 + (ce - c));
      const float *app = ap + p * g.delta_pstride, *wpp = wp + p * g.theta_pstride;
      pyz_steps4_all(
          c0, c1, acc,
          [&](int cc, float4 &a4, float4 &b4) {
            const int k = 8 * cc + 4 * h;
            a4 = *reinterpret_cast<const float4 *>(app + k);
            b4 = *reinterpret_cast<const float4 *>(wpp + k);
          },
          PyzNoUse4());
      c += c1 - c0;
    }
  }
  {   // dword steps: all of n when the float4 rule fails, else the tail past the last whole chunk of 8
    const int t0 = 8 * c8, steps = (N - t0 + 1) >> 1;
    const int T = g.P * steps;
    int s = (int)(((long long)T * w) / S);
    const int se = (int)(((long long)T * (w + 1)) / S);
    while (s < se) {
      const int p = s / steps, s0 = s - p * steps, s1 = min(steps, s0 + (se - s));
      const float *app = ap + p * g.delta_pstride, *wpp = wp + p * g.theta_pstride;
      pyz_steps1_all(
          s0, s1, acc,
          [&](int ss, float &a, float &b) {
            const int kk = t0 + 2 * ss + h;
            const int kc = kk < N ? kk : 0;
            a = app[kc];
            b = wpp[kc];
          },
          [&](int ss, float &a, float &b) {
            const bool vk = t0 + 2 * ss + h < N;
            a = vk ? a : 0.0f;
            b = vk ? b : 0.0f;
          });
      s += s1 - s0;
    }
  }
  const float scale = g.scale, eps = g.eps;
  const int accumulate = g.accumulate;
  float *out = g.out, *xadv = g.xadv;
  const float *x = g.x;
  pyz_tile_epilogue(acc, red, [&](int ro, int co, float v) {
    const int mm = m0 + ro, jj = j0 + co;
    if (mm < rows && jj < K) {
      const long long o = (long long)mm * K + jj;
      float gv = scale * v;
      if (accumulate) gv = out[o] + gv;
      out[o] = gv;
      if (xadv) {   // np.sign: 0 stays 0, NaN stays NaN
        const float sg = gv > 0.0f ? 1.0f : (gv < 0.0f ? -1.0f : gv);
        xadv[o] = x[o] + eps * sg;
      }
    }
  });
}

// draws per launch the kernel's 32-bit step counters take (P * N / 2 steps, P * N / 8 chunks)
static inline int pyz_input_grad_max_draws(int N) { return std::max(1, (1 << 30) / std::max(N, 1)); }

static inline void pyz_launch_input_grad(const InputGradArgs &g, hipStream_t st) {
  const long long tiles = (long long)((g.rows + 31) / 32) * ((g.K + 31) / 32);
  const int S = pyz_pick_waves(tiles, (long long)g.P * g.N / 2);
  PYZ_LAUNCH(k_input_grad, dim3((unsigned)tiles), dim3(64 * S), S > 1 ? S * 4096 : 0, st, g);
}
