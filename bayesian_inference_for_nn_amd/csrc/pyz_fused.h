// pyz_fused.h -- fused kernels that cut a gradient step down to three launches.
//
// Every kernel of this path is latency-bound (the 784->200->10 step is
// 654 MFLOP / 7 MB, all L2 resident), so what counts is the number of launches and of
// dependent memory round trips, not FLOP/s.  A step of an L-layer MLP is
//     k_dense_fwd            x (L-1)   hidden layers
//     k_head                 x 1       last layer + loss + delta_L + delta_{L-1}
//     k_dense_bwd_data       x (L-2)   remaining data gradients
//     k_wgrad_all            x 1       every layer's [dW; db] + the optimizer update
// i.e. 3 launches for the 2-layer headline model instead of 7.
#pragma once

#include <type_traits>

#include "pyz_common.h"
#include "pyz_gemm.h"
#include "pyz_kernels.h"

// ---------------------------------------------------------------- head
// One workgroup (4 waves) owns 32 batch rows of the LAST Dense layer (N <= 32):
//   1. z = h_in W + b           (MFMA, the 4 waves split K, LDS combine)
//   2. loss row terms, delta_L  (SparseCategoricalCrossentropy / MeanSquaredError as
//                                in k_loss_scce / k_loss_mse: Dataset.py:152-159)
//   3. delta_{L-1} = (delta_L W^T) * act'(h_in)   (MFMA with delta_L from LDS)
// (Field order: what k_head_rows reads in front of its first operand load fills the first two 64-byte lines and is asked
// for in one trip, see DenseArgs.)
struct HeadArgs {
  // ---- line 0
  const float *hin;          // (P, max_batch, K) input of the last layer, or the data x when L == 1
  long long hin_pstride;
  const float *theta;
  long long theta_pstride;
  long long w_off;
  const StepCtl *ctl;
  const int32_t *row_idx;    // gather of hin rows (only when hin is the data, L == 1) and of the labels
  const StepCtl *gate;       // when set: nothing happens on steps with gate->n % gate_mod == 0 (see DenseArgs)
  // ---- line 1
  const void *y;
  double *part;              // (P, nblk) per-workgroup sums of the row losses
  int lda;
  int K, N;
  int loss;
  int gather_hin;
  int gate_mod;
  int init_on;
  int nblk;
  int act_last, act_prev, vec;
  int wt;                    // write-through stores for the outputs (pyz_st)
  // ---- the rest
  float *out_last;           // optional (P, max_batch, N): logits (softmax layer) / outputs
  float *delta_last;         // (P, max_batch, N) or nullptr (loss only)
  float *delta_prev;         // (P, max_batch, K) or nullptr
  long long last_pstride, prev_pstride;
  StepCtl init;              // the step scalars by value when the head is the first kernel of an eager step (L == 1)
  // k_head_rows behind a split-reduction forward (k_dense_fwd_ring, k_split): the hidden layer arrives as n_hparts <= 8 raw
  // partial sums (hparts + s * hpart_stride + row * K + unit); the head adds them in split order, then the hidden layer's
  // bias (bias_prev[unit]) and activation (act_prev), and stores the row of activations to h_store for the weight gradients
  const float *hparts;
  int n_hparts;
  long long hpart_stride;
  const float *bias_prev;
  float *h_store;
};

// lanes 8q..8q+7 of a wave cooperate on one row: reductions over the 8-lane group
__device__ __forceinline__ float pyz_grp8_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64));
  v = fmaxf(v, __shfl_xor(v, 2, 64));
  return fmaxf(v, __shfl_xor(v, 4, 64));
}
__device__ __forceinline__ float pyz_grp8_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v + __shfl_xor(v, 4, 64);
}

// blockDim.x = 64 * S with S in {4, 8}; dynamic LDS = S * 4096 + 2 * 32 * 33 * 4 + 64 bytes
__global__ void __launch_bounds__(512) k_head(HeadArgs g) {
  extern __shared__ float lds[];
  PYZ_STAMP(1, 0);
  const int S = blockDim.x >> 6, w = pyz_wave_id(), l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  if (g.gate && g.gate->n % g.gate_mod == 0) return;
  float *red = lds, *zt = lds + S * 1024, *dt = zt + 32 * 33;
  double *lsum = reinterpret_cast<double *>(dt + 32 * 33);  // 4 doubles (8-byte aligned: S*4096 + 8448 bytes)
  const StepCtl ctl = pyz_ctl_first(g.ctl, g.init, g.init_on);
  const int batch = ctl.batch, p = blockIdx.y, m0 = blockIdx.x * 32;
  if (m0 >= batch) {
    if (threadIdx.x == 0) g.part[p * g.nblk + blockIdx.x] = 0.0;
    return;
  }
  const int K = g.K, N = g.N;
  const int32_t *idx = g.row_idx ? g.row_idx + ctl.row_off : nullptr;
  // loss-phase inputs (threads 0..255: row = t >> 3), fetched now so their latency hides behind phase 1
  const int lrow = threadIdx.x >> 3, lsub = threadIdx.x & 7;
  const int lmm = m0 + lrow;
  const bool lvalid = threadIdx.x < 256 && lmm < batch;
  long long yrow = min(lmm, batch - 1);
  if (idx) yrow = idx[yrow];
  int ylab = 0;
  if (g.loss == PYZ_LOSS_SCCE) ylab = reinterpret_cast<const int32_t *>(g.y)[yrow];
  // delta_{L-1} operands of this wave's tile (jt = w): the act' inputs and the W rows depend on nothing
  // computed here, so they are fetched now and their latency hides behind phases 1 and 2
  const int tiles_j = (K + 31) >> 5;
  const int nsteps = (N + 1) >> 1;  // <= 16 (N <= 32)
  const float *wl = g.theta + p * g.theta_pstride + g.w_off;
  const float *hp = g.hin + p * g.hin_pstride;
  const bool pre = g.delta_prev && w < tiles_j && !g.gather_hin;
  float hv0[16], bw0[16];
  if (pre) {
    const int j = min(w * 32 + r, K - 1);
    const float *wp = wl + (long long)j * N;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int mm = min(m0 + (i & 3) + 8 * (i >> 2) + 4 * h, batch - 1);
      hv0[i] = hp[(long long)mm * K + j];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int kk = 2 * q + h;
      bw0[q] = (q < nsteps) ? wp[kk < N ? kk : 0] : 0.0f;
    }
  }
  {
    const int m = min(m0 + r, batch - 1), n = min(r, N - 1);
    long long row = m;
    if (g.gather_hin && idx) row = idx[m];
    const float *ap = g.hin + p * g.hin_pstride + row * g.lda;
    f32x16 acc = {0};
    PYZ_STAMP(1, 1);
    pyz_fwd_accumulate(acc, ap, wl, n, K, N, g.vec, w, S, h);
    PYZ_STAMP(1, 2);
    float *my = red + w * 1024;
#pragma unroll
    for (int i = 0; i < 16; ++i) my[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[i];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 1024; e += blockDim.x) {
    float v = red[e];
    for (int ww = 1; ww < S; ++ww) v += red[ww * 1024 + e];
    zt[(e >> 5) * 33 + (e & 31)] = v;
  }
  __syncthreads();
  PYZ_STAMP(1, 3);
  // ---- loss rows: 8 lanes per row, classes c = lsub, lsub + 8, ... (N <= 32)
  if (threadIdx.x < 256) {
    const float *z = zt + lrow * 33;
    float *d = dt + lrow * 33;
    float *ol = g.out_last ? g.out_last + p * g.last_pstride + (long long)lmm * N : nullptr;
    float *dl = g.delta_last ? g.delta_last + p * g.last_pstride + (long long)lmm * N : nullptr;
    float zv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) zv[q] = (lsub + 8 * q < N) ? z[lsub + 8 * q] : 0.0f;
    float lm = 0.0f;
    if (g.loss == PYZ_LOSS_SCCE) {
      float mx = -3.0e38f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (lsub + 8 * q < N) mx = fmaxf(mx, zv[q]);
      mx = pyz_grp8_max(mx);
      float se = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (lsub + 8 * q < N) se += expf(zv[q] - mx);
      se = pyz_grp8_sum(se);
      const float lse = mx + logf(se);
      const float zy = (ylab >= 0 && ylab < N) ? z[ylab] : __builtin_nanf("");
      lm = lse - zy;
      const float inv = 1.0f / (float)batch;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = lsub + 8 * q;
        if (c < N) {
          const float dv = lvalid ? (expf(zv[q] - lse) - (c == ylab ? 1.0f : 0.0f)) * inv : 0.0f;
          d[c] = dv;
          if (lvalid && dl) dl[c] = dv;
          if (lvalid && ol) ol[c] = zv[q];
        }
      }
    } else if (g.loss == PYZ_LOSS_BCE) {
      // one sigmoid unit (N == 1: pyz_mlp_create), from its logit: the row's first lane has it
      if (lsub == 0) {
        const float yv = reinterpret_cast<const float *>(g.y)[yrow];
        float o;
        lm = pyz_bce_row(zv[0], yv, o);
        const float dv = lvalid ? (o - yv) * (1.0f / (float)batch) : 0.0f;
        d[0] = dv;
        if (lvalid && dl) dl[0] = dv;
        if (lvalid && ol) ol[0] = o;
      }
    } else {
      const float *y = reinterpret_cast<const float *>(g.y) + yrow * N;
      const float sc = 2.0f / ((float)batch * (float)N);
      float a = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = lsub + 8 * q;
        if (c < N) {
          const float o = pyz_act(zv[q], g.act_last);
          const float e = o - y[c];
          a += e * e;
          const float dv = lvalid ? sc * e * pyz_act_grad(o, g.act_last) : 0.0f;
          d[c] = dv;
          if (lvalid && dl) dl[c] = dv;
          if (lvalid && ol) ol[c] = o;
        }
      }
      lm = pyz_grp8_sum(a) / (float)N;
    }
    const double ws = pyz_wave_sum((lvalid && lsub == 0) ? (double)lm : 0.0);
    if (l == 0) lsum[w] = ws;
  }
  __syncthreads();
  if (threadIdx.x == 0) g.part[p * g.nblk + blockIdx.x] = (lsum[0] + lsum[1]) + (lsum[2] + lsum[3]);
  PYZ_STAMP(1, 4);
  if (!g.delta_prev) return;
  // ---- delta_{L-1} tile by tile: (delta_L [32 x N]) (W^T [N x 32]) * act'(h_in)
  float *op = g.delta_prev + p * g.prev_pstride;
  for (int jt = w; jt < tiles_j; jt += S) {
    const int j0 = jt * 32, jj = j0 + r, j = min(jj, K - 1);
    const float *wp = wl + (long long)j * N;
    float hv[16];
    f32x16 acc = {0};
    if (pre && jt == w) {  // operands already in registers
#pragma unroll
      for (int i = 0; i < 16; ++i) hv[i] = hv0[i];
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (q < nsteps) {
          const int kk = 2 * q + h;
          const bool vk = kk < N;
          const float a = vk ? dt[r * 33 + kk] : 0.0f;
          acc = pyz_mfma(a, vk ? bw0[q] : 0.0f, acc);
        }
      PYZ_STAMP(1, 6);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int mm = min(m0 + (i & 3) + 8 * (i >> 2) + 4 * h, batch - 1);
        long long row = mm;
        if (g.gather_hin && idx) row = idx[mm];
        hv[i] = hp[row * K + j];
      }
      pyz_steps1_all(
          0, nsteps, acc,
          [&](int s, float &a, float &b) {
            const int kk = 2 * s + h;
            const int kc = kk < N ? kk : 0;
            a = dt[r * 33 + kc];
            b = wp[kc];
          },
          [&](int s, float &a, float &b) {
            const bool vk = 2 * s + h < N;
            a = vk ? a : 0.0f;
            b = vk ? b : 0.0f;
          });
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int mm = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (mm < batch && jj < K) op[(long long)mm * K + jj] = acc[i] * pyz_act_grad(hv[i], g.act_prev);
    }
  }
  PYZ_STAMP(1, 5);
}

// ---------------------------------------------------------------- head, one wave per batch row
// The last layer of these models is narrow (N <= 32 classes / outputs) and its input a few hundred
// wide: 32 rows x K x N per workgroup is too little for the MFMA path above to amortise its LDS
// combines and barriers (k_head: 7.7 us in-kernel on 32 CUs for the 784->200->10 step).  Here every
// WAVE owns ONE batch row and the grid covers the whole chip (batch/4 workgroups of 4 waves):
// lane l holds hidden units l, l+64, ... (UT of them) and their W rows in registers, so
//   z      = sum over the lane's units, then a butterfly sum over the 64 lanes (fixed order),
//   loss row, delta_L           every lane redundantly (N <= 32 values),
//   delta_{L-1}[u] = act'(h[u]) * sum_c delta_L[c] W[u][c]   for the lane's own units,
// with no LDS, no barrier and coalesced row loads / stores.  NP = padded class count.
// value of lane `lane` (compile-time or wave-uniform) as a scalar
__device__ __forceinline__ float pyz_readlane(const float v, const int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// every lane of a 16-lane row gets the row's sum: lane ^ 1, lane ^ 2 (quad permutes), then the
// mirror inside each half row and the mirror of the row (data-parallel primitives: VALU speed)
template <int CTRL>
__device__ __forceinline__ float pyz_dpp(const float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float pyz_row16_allsum(float v) {
  v += pyz_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += pyz_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += pyz_dpp<0x141>(v);  // row_half_mirror
  v += pyz_dpp<0x140>(v);  // row_mirror
  return v;
}

__device__ __forceinline__ float pyz_row16_allmax(float v) {
  v = fmaxf(v, pyz_dpp<0xB1>(v));
  v = fmaxf(v, pyz_dpp<0x4E>(v));
  v = fmaxf(v, pyz_dpp<0x141>(v));
  v = fmaxf(v, pyz_dpp<0x140>(v));
  return v;
}

// The lane-resident part of the last layer's [W; b]: lane l keeps the rows of units l, l + 64, ... and (lane c) b[c].
// A wave loads it once and uses it for every batch row it takes.
template <int UT, int NP>
struct PyzHeadW {
  float wv[UT][NP];
  float bias_mine;
};

template <int UT, int NP>
__device__ __forceinline__ void pyz_head_load_w(const HeadArgs &g, const int p, const int l, PyzHeadW<UT, NP> &W) {
  const int K = g.K, N = g.N;
  const float *wl = g.theta + p * g.theta_pstride + g.w_off;
  // Operands through buffer descriptors (per-lane byte offsets, range checked against the byte count).
  // Only the per-lane offset is range checked by the hardware (not the scalar one): units past K get an
  // out-of-range voffset; a padded class c >= N reads a neighbouring in-range element (or 0 past the
  // end), which is harmless: z[c] is never used and delta_L[c] = 0 multiplies it
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(wl), 0, (K + 1) * N * 4, 0x00020000);
  constexpr unsigned OOB = 0x7FFFFF00u;
#pragma unroll
  for (int t = 0; t < UT; ++t) {
    const int u = l + 64 * t;
    const unsigned wo = u < K ? 4u * (unsigned)u * (unsigned)N : OOB;
#pragma unroll
    for (int c = 0; c < NP; ++c) W.wv[t][c] = pyz_buf_load(rw, wo + 4u * (unsigned)c, 0u);
  }
  W.bias_mine = pyz_buf_load(rw, l < N ? 4u * ((unsigned)K * (unsigned)N + (unsigned)l) : OOB, 0u);  // lane c: b[c]
}

// the lane's units of input row `hrow` (units past K read as zero)
template <int UT>
__device__ __forceinline__ void pyz_head_load_h(const HeadArgs &g, const int p, const long long hrow, const int l, float (&hv)[UT]) {
  const float *hp = g.hin + p * g.hin_pstride + hrow * g.lda;
  const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(hp), 0, g.K * 4, 0x00020000);
#pragma unroll
  for (int t = 0; t < UT; ++t) hv[t] = pyz_buf_load(rh, 4u * (unsigned)(l + 64 * t), 0u);
}

// The head of ONE batch row m by ONE wave (lane l).  PRELOADED: W already holds the wave's share of [W; b] (several
// rows per wave); else it is fetched here, behind the row's own loads (one row per wave: the order of round 1 --
// with the 48 strided [W; b] loads in front of them the row's input and label chain start 0.4 us later).
// HP: the hidden layer arrives as the partial sums of a split-reduction forward (g.hparts; only instantiated for the shapes
// that path takes -- as a run-time branch it cost every instantiation 35 registers: k_head_rows<4, 12, 4> fell from four to
// three waves per SIMD and from 60 to 76 us at C5)
template <int UT, int NP, bool PRELOADED, bool HP = false>
__device__ __forceinline__ void pyz_head_row(const HeadArgs &g, const int batch, const long long row_off, const int p,
                                             const int m, const int l, PyzHeadW<UT, NP> &W) {
  const int K = g.K, N = g.N;
  int yidx = m;   // the row's index in the data set: requested here, waited for where the label is loaded (below)
  if (g.row_idx) yidx = g.row_idx[row_off + m];
  // The class loops below are straight-line code over the NP padded
  // classes: no per-class branches (conditional writes into the register arrays would turn them
  // into whole-vector copies).
  float hv[UT], z[NP];
  if constexpr (HP) {
    // the hidden layer as raw partial sums of a split reduction: eight loads per unit in flight together (splits past
    // n_hparts are out of range: zero), summed in split order; then bias and activation; the row goes to h_store
    const float *pp = g.hparts + (long long)m * K;
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pp), 0,
        (int)(((long long)(g.n_hparts - 1) * g.hpart_stride + K) * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.bias_prev), 0, K * 4, 0x00020000);
    constexpr unsigned OOBH = 0x7FFFFF00u;
    float pv[UT][8], bv[UT];
#pragma unroll
    for (int t = 0; t < UT; ++t) {
      const int u = l + 64 * t;
#pragma unroll
      for (int sp = 0; sp < 8; ++sp)
        pv[t][sp] = pyz_buf_load(rp, (u < K && sp < g.n_hparts) ? 4u * (unsigned)(sp * g.hpart_stride + u) : OOBH, 0u);
      bv[t] = pyz_buf_load(rb, 4u * (unsigned)u, 0u);
    }
#pragma unroll
    for (int t = 0; t < UT; ++t) {
      float a = pv[t][0];
#pragma unroll
      for (int sp = 1; sp < 8; ++sp) a += pv[t][sp];
      hv[t] = pyz_act(a + bv[t], g.act_prev);
      const int u = l + 64 * t;
      if (u < K) pyz_st(g.h_store + (long long)m * K + u, hv[t], g.wt);
    }
  } else {
    // A branch, not `gather_hin ? index : m`: behind the select the row's loads (and the 48 loads of [W; b] behind them)
    // waited for the row index, which only a gathered input (L == 1) and the label need.
    if (g.gather_hin) {
      asm volatile("; gathered input: the row index is needed here" ::: "memory");   // (keeps this a branch)
      // (made scalar HERE: left to the compiler, the two arms become one load behind a select of the row, and the scalar
      //  copy of the index -- with its wait -- moves back to where the index was loaded)
      pyz_head_load_h<UT>(g, p, __builtin_amdgcn_readfirstlane(yidx), l, hv);
    } else {
      pyz_head_load_h<UT>(g, p, m, l, hv);
    }
  }
  if (!PRELOADED) pyz_head_load_w<UT, NP>(g, p, l, W);
  const auto &wv = W.wv;
  const float bias_mine = W.bias_mine;
  // The index is wave-uniform, and as a scalar it is waited for where it was loaded (readfirstlane), in front of every
  // operand load above, whatever the branch says.  From here on it is a per-lane value: the label is loaded through a
  // vector address and the wait for the index stands here, behind the row's and [W; b]'s loads.
  asm volatile("; the row index arrives here" : "+v"(yidx));
  const long long yrow = yidx;
  int ylab = 0;
  if (g.loss == PYZ_LOSS_SCCE) ylab = reinterpret_cast<const int32_t *>(g.y)[yrow];
  PYZ_STAMP(1, 1);
  // ---- z[c] = sum_u h[u] W[u][c] + b[c]: the lane's units, then a butterfly over the lanes
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    float a = 0.0f;
#pragma unroll
    for (int t = 0; t < UT; ++t) a = fmaf(hv[t], wv[t][c], a);
    z[c] = a;
  }
  // sum over the 64 lanes without LDS traffic: four DPP steps leave each 16-lane row's sum in all its
  // lanes, the four row sums are read as scalars and added in a fixed order (bitwise reproducible)
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    const float v = pyz_row16_allsum(z[c]);
    z[c] = ((pyz_readlane(v, 0) + pyz_readlane(v, 16)) + (pyz_readlane(v, 32) + pyz_readlane(v, 48))) + pyz_readlane(bias_mine, c);
  }
  PYZ_STAMP(1, 2);
  // ---- loss row and delta_L (every lane holds all N values; padded classes carry zeros)
  float d2[NP], lm, my_d = 0.0f, my_o = 0.0f;
  if (g.loss == PYZ_LOSS_SCCE && NP <= 16) {
    // softmax with the classes spread over the lanes of each 16-lane row (lane c owns class c; the four rows
    // hold copies): one exp per lane instead of N in sequence on every lane, max and sum by DPP row steps
    const int lc = l & 15;
    float zc = z[0];
#pragma unroll
    for (int c = 1; c < NP; ++c) zc = (lc == c) ? z[c] : zc;
    const bool on = lc < N;
    const float mx = pyz_row16_allmax(on ? zc : -3.0e38f);
    const float exv = on ? expf(zc - mx) : 0.0f;
    const float se = pyz_row16_allsum(exv);
    const float lse = mx + logf(se);
    const bool mine = on && lc == ylab;
    float zy = pyz_row16_allsum(mine ? zc : 0.0f);
    zy = (ylab >= 0 && ylab < N) ? zy : __builtin_nanf("");
    const float inv = 1.0f / (float)batch, rse = 1.0f / se;
    my_d = (exv * rse - (mine ? 1.0f : 0.0f)) * inv;  // softmax - onehot, over the batch mean (0 past N)
    my_o = zc;
#pragma unroll
    for (int c = 0; c < NP; ++c) d2[c] = pyz_readlane(my_d, c < 16 ? c : 0);
    lm = lse - zy;
  } else {
    float outv[NP];
    if (g.loss == PYZ_LOSS_SCCE) {
      float mx = -3.0e38f;
#pragma unroll
      for (int c = 0; c < NP; ++c) mx = fmaxf(mx, c < N ? z[c] : -3.0e38f);
      float ex[NP], se = 0.0f;
#pragma unroll
      for (int c = 0; c < NP; ++c) {
        ex[c] = c < N ? expf(z[c] - mx) : 0.0f;
        se += ex[c];
      }
      const float lse = mx + logf(se);
      float zy = __builtin_nanf("");
      const float inv = 1.0f / (float)batch, rse = 1.0f / se;
#pragma unroll
      for (int c = 0; c < NP; ++c) {
        zy = (c == ylab && c < N) ? z[c] : zy;
        d2[c] = (ex[c] * rse - ((c == ylab && c < N) ? 1.0f : 0.0f)) * inv;  // softmax - onehot, over the batch mean
        outv[c] = z[c];
      }
      lm = lse - zy;
    } else if (NP == 4 && g.loss == PYZ_LOSS_BCE) {
      // one sigmoid unit (N == 1: pyz_mlp_create; only the narrowest padding carries the arm), from its logit
      const float yv = reinterpret_cast<const float *>(g.y)[yrow];
      float o;
      lm = pyz_bce_row(z[0], yv, o);
      const float dv = (o - yv) * (1.0f / (float)batch);
#pragma unroll
      for (int c = 0; c < NP; ++c) {
        d2[c] = c == 0 ? dv : 0.0f;
        outv[c] = c == 0 ? o : 0.0f;
      }
    } else {
      const float *y = reinterpret_cast<const float *>(g.y) + yrow * N;
      const float sc = 2.0f / ((float)batch * (float)N);
      const int act = g.act_last;
      float a = 0.0f;
#pragma unroll
      for (int c = 0; c < NP; ++c) {
        const float o = pyz_act(z[c], act);
        const float e = o - y[min(c, N - 1)];
        a += c < N ? e * e : 0.0f;
        d2[c] = c < N ? sc * e * pyz_act_grad(o, act) : 0.0f;
        outv[c] = o;
      }
      lm = a / (float)N;
    }
    // lane c stores column c of the row
#pragma unroll
    for (int c = 0; c < NP; ++c) {
      my_d = (l == c) ? d2[c] : my_d;
      my_o = (l == c) ? outv[c] : my_o;
    }
  }
  PYZ_STAMP(1, 3);
  if (l < N) {
    if (g.out_last) pyz_st(g.out_last + p * g.last_pstride + (long long)m * N + l, my_o, g.wt);
    if (g.delta_last) pyz_st(g.delta_last + p * g.last_pstride + (long long)m * N + l, my_d, g.wt);
  }
  if (l == 0) g.part[p * g.nblk + m] = (double)lm;
  PYZ_STAMP(1, 4);
  if (!g.delta_prev) return;
  float *op = g.delta_prev + p * g.prev_pstride + (long long)m * K;
  const int actp = g.act_prev;
#pragma unroll
  for (int t = 0; t < UT; ++t) {
    const int u = l + 64 * t;
    float a = 0.0f;
#pragma unroll
    for (int c = 0; c < NP; ++c) a = fmaf(d2[c], wv[t][c], a);
    if (u < K) pyz_st(op + u, a * pyz_act_grad(hv[t], actp), g.wt);
  }
  PYZ_STAMP(1, 5);
}

// RW = batch rows per wave: 1 when the launch has few rows (a single chain: every row its own wave, the chip is
// barely filled as it is), 4 when there are tens of thousands (64 particles x 1024 rows): the wave's share of
// [W; b] -- UT x NP strided loads, most of the kernel's memory instructions -- is then fetched once for four rows.
template <int UT, int NP, int RW = 1, bool HP = false>
__global__ void __launch_bounds__(256) k_head_rows(HeadArgs g) {
  PYZ_STAMP(1, 0);
  const int w = pyz_wave_id(), l = threadIdx.x & 63;
  // the first two lines of the arguments in one trip, the gate test out of the same answer (see k_dense_fwd)
  asm volatile("; arguments in one trip" ::"s"(g.hin), "s"(g.hin_pstride), "s"(g.theta), "s"(g.theta_pstride), "s"(g.w_off),
               "s"(g.ctl), "s"(g.row_idx), "s"(g.gate), "s"(g.y), "s"(g.part), "s"(g.lda), "s"(g.K), "s"(g.N), "s"(g.loss),
               "s"(g.gather_hin), "s"(g.gate_mod), "s"(g.init_on), "s"(g.nblk), "s"(g.act_last), "s"(g.act_prev), "s"(g.vec),
               "s"(g.wt));
  if (g.gate && g.gate->n % g.gate_mod == 0) return;
  // The step scalars: a branch, not pyz_ctl_first's select -- the select asks for the 40 bytes of g.init (another trip to
  // the argument segment, in front of the operand loads) in every launch, the branch only where the head is the first
  // kernel of an eager step.
  StepCtl ctl;
  if (g.init_on) {
    asm volatile("; the step scalars by value" ::: "memory");   // (keeps this a branch)
    ctl = pyz_ctl_first(g.ctl, g.init, 1);
  } else {
    // both scalars with one wait, here: a row offset still in flight at the batch test stays "pending" on the path
    // without a row table, and the register it would land in is then waited for in the middle of the operand loads
    const PyzCtlHot c = pyz_ctl_arrived(pyz_ctl_request(g.ctl));
    ctl.batch = c.batch;
    ctl.row_off = c.row_off;
  }
  const int batch = ctl.batch, p = blockIdx.y;
  const int m0 = (blockIdx.x * 4 + w) * RW;  // this wave's first batch row (scalar)
  if (m0 >= batch) {
    if (l < RW && m0 + l < g.nblk) g.part[p * g.nblk + m0 + l] = 0.0;
    return;
  }
  PyzHeadW<UT, NP> W;
  if (RW == 1) {
    pyz_head_row<UT, NP, false, HP>(g, batch, ctl.row_off, p, m0, l, W);
    return;
  }
  pyz_head_load_w<UT, NP>(g, p, l, W);
#pragma unroll 1
  for (int rr = 0; rr < RW; ++rr) {
    const int m = m0 + rr;
    if (m >= batch) {   // uniform
      if (l == 0 && m < g.nblk) g.part[p * g.nblk + m] = 0.0;
      continue;
    }
    pyz_head_row<UT, NP, true>(g, batch, ctl.row_off, p, m, l, W);
  }
}

// ---------------------------------------------------------------- the next step's batch, assembled ahead of its step
// In a device-resident run the rows of step s + 1 are known while step s runs (row table + per-run tables).  The
// workgroups of k_wgrad_all that own no tile -- 73 of the 256 CUs idle at C2 -- copy those rows of the resident data
// set into the other one of two contiguous (max_batch, K) buffers.  The forward pass of step s + 1 then reads plain
// contiguous rows: no index load in front of its first operand load, no first touch of HBM rows on its critical
// path, no copy to store for the weight-gradient kernel.  A worker takes rows that the forward tiles of workgroups
// with its own blockIdx % 8 read (workgroups are dealt round-robin over the XCDs: the copy then waits in the L2 of
// the XCD that reads it; placement only changes speed).
struct PrepArgs {
  const float *src;           // (n_rows, lda) resident data set; nullptr: no preparation in this launch
  float *dst;                 // (max_batch, K) contiguous batch of the NEXT step
  const int32_t *row_idx;     // the run's row table
  const int32_t *tab_bs;      // per-run batch sizes
  long long row_stride;
  int K, lda;
  int fwd_tiles, fwd_tiles_n; // tile grid of the forward kernel that will read dst (pyz_xcd_remap over fwd_tiles ids)
};

// The image form of the next batch (pyz_prep_rows<true>; SGD / SGLD / SWAG / BBB runs with K % 8 == 0): instead of the
// row-major copy the workers leave the batch twice, each time in the order the MFMA fragments of its reader want it, in
// 1 KiB blocks of 64 pieces of 16 bytes -- piece l is what lane l of the reading wave loads, so one wave-instruction
// covers eight whole 128-byte lines.  With mb = row_stride (the plan's max_batch), RB = ceil(mb / 32), C8 = K / 8,
// KB = ceil(K / 32), G = ceil(mb / 8):
//   forward image, at dst, RB x C8 blocks: block (rb, c), piece r + 32 h = X[32 rb + r][8 c + 4 h .. + 3]
//       float offset (((rb C8 + c) 2 + h) 32 + r) 4 + q                     (k_dense_fwd_frag)
//   weight-gradient image, at dst + 32 RB K, KB x G blocks: block (kb, g), piece i + 32 h = column 32 kb + i of rows
//       8 g + h + {0, 2, 4, 6}: that lane's A values of the MFMA steps 4 g .. 4 g + 3
//       float offset (((kb G + g) 2 + h) 32 + i) 4 + q                      (k_wgrad_all_frag, layer 0)
// Columns at or past K of the last column block are zeros; rows at or past the batch hold nothing defined (both readers
// select them away).
__device__ __forceinline__ long long pyz_frag_fwd_floats(const int mb, const int K) { return (long long)((mb + 31) >> 5) * 32 * K; }

// the row groups of eight that begin in rows [ra, rb) of the batch of nb rows, as both images (the workers' shares are
// consecutive ranges of [0, nb): every group has one owner).  A wave takes one row group of one column block at a time, eight rows x 32 columns: lane (r8, c) loads the 16 bytes of columns 4 c .. 4 c + 3 of row 8 g + r8 -- whole
// 128-byte lines of eight source rows -- and stores them as they are, a piece of the forward image: the eight lanes of a c
// fill one line.  The four lanes (h + 2 q, c), q = 0 .. 3, then transpose their 4 x 4 values among themselves (four lane
// permutes), which leaves each of them one piece of the weight-gradient image, and the wave stores that block's whole KiB
// in one instruction.  No store leaves part of a line to a later one (they are write-through), and the loads of four such
// units are in flight before the first store.
__device__ __forceinline__ void pyz_copy_rows_frag(const PrepArgs &g, const int32_t *idx, const int ra, const int rb, const int nb) {
  const int ga = (ra + 7) >> 3, gb = (rb + 7) >> 3;
  if (ga >= gb) return;
  const int K = g.K, K4 = K >> 2, C8 = K >> 3, KB = (K + 31) >> 5;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int r8 = lane & 7, cl = lane >> 3, h = r8 & 1, qd = r8 >> 1;
  const int mb = (int)g.row_stride, G = (mb + 7) >> 3;
  float *fimg = g.dst, *wimg = g.dst + pyz_frag_fwd_floats(mb, K);
  const int total = (gb - ga) * KB;                       // units: (row group, column block)
  for (int u0 = wv; u0 < total; u0 += 4 * nw) {           // (uniform per wave)
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int unit = min(u0 + u * nw, total - 1), gi = ga + unit / KB, c4 = 8 * (unit % KB) + cl;
      const int m = min(8 * gi + r8, nb - 1);             // (rows past the batch, columns past K: any defined element)
      v[u] = *reinterpret_cast<const float4 *>(g.src + (long long)idx[m] * g.lda + 4 * min(c4, K4 - 1));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int unit = u0 + u * nw;
      if (unit >= total) break;
      const int gi = ga + unit / KB, kb = unit % KB, c4 = 8 * kb + cl, m = 8 * gi + r8;
      const bool vc = c4 < K4;
      if (vc && m < nb) {
        float *d = fimg + ((((long long)(m >> 5) * C8 + (c4 >> 1)) * 2 + (c4 & 1)) * 32 + (m & 31)) * 4;
        const f32x4 vv = {v[u].x, v[u].y, v[u].z, v[u].w};
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(d), "v"(vv) : "memory");   // (write-through: see pyz_copy_rows)
      }
      // round k: lane q sends its column (q + k) % 4; lane qd takes from lane (qd - k) % 4 that lane's column qd, its row's value
      const float x0 = vc ? v[u].x : 0.0f, x1 = vc ? v[u].y : 0.0f, x2 = vc ? v[u].z : 0.0f, x3 = vc ? v[u].w : 0.0f;
      float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, o3 = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int js = (qd + k) & 3, qs = (qd - k) & 3;
        const float send = js == 0 ? x0 : (js == 1 ? x1 : (js == 2 ? x2 : x3));
        const float got = __shfl(send, (cl << 3) | (2 * qs + h), 64);
        o0 = qs == 0 ? got : o0;
        o1 = qs == 1 ? got : o1;
        o2 = qs == 2 ? got : o2;
        o3 = qs == 3 ? got : o3;
      }
      float *dw = wimg + ((((long long)kb * G + gi) * 2 + h) * 32 + 4 * cl + qd) * 4;
      const f32x4 ww = {o0, o1, o2, o3};
      asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dw), "v"(ww) : "memory");
    }
  }
}

// rows [ra, rb) of the batch whose row indices start at idx: dst[m][:] = src[idx[m]][:]
__device__ __forceinline__ void pyz_copy_rows(const PrepArgs &g, const int32_t *idx, const int ra, const int rb) {
  const int K = g.K, nt = blockDim.x, t = threadIdx.x;
  if (ra >= rb) return;
  if ((K & 3) == 0 && (g.lda & 3) == 0 && ((reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst)) & 15) == 0) {
    const int K4 = K >> 2, total = (rb - ra) * K4;
    for (int e0 = t; e0 < total; e0 += 4 * nt) {   // four independent 16-byte loads per thread and trip
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = min(e0 + u * nt, total - 1), m = ra + e / K4, c = e % K4;
        v[u] = *reinterpret_cast<const float4 *>(g.src + (long long)idx[m] * g.lda + 4 * c);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * nt;
        if (e < total) {
          float *d = g.dst + (long long)(ra + e / K4) * K + 4 * (e % K4);
          // write-through (sc1) stores: the copy leaves L2 while the tile workgroups still run.  With plain stores the
          // 3.2 MB stay dirty in L2 until the kernel ends and its end waits for their write-back (measured at C2:
          // k_wgrad_all 10.75 against 10.3 us; the stand-alone first-batch launch 28 against 4 us)
          const f32x4 vv = {v[u].x, v[u].y, v[u].z, v[u].w};
          asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(d), "v"(vv) : "memory");
        }
      }
    }
    return;
  }
  const int total = (rb - ra) * K;
  for (int e = t; e < total; e += nt) {
    const int m = ra + e / K, c = e % K;
    g.dst[(long long)m * K + c] = g.src[(long long)idx[m] * g.lda + c];
  }
}

// worker j of cnt (its workgroup id is bid): its share of the nb rows.  FRAG: as the two images (the row groups that begin
// in the share)
template <bool FRAG = false>
__device__ __forceinline__ void pyz_prep_rows(const PrepArgs &g, const int32_t *idx, const int nb, const int j, const int cnt,
                                              const int bid) {
  int ra, rb;
  if (cnt >= 8 && g.fwd_tiles >= 8) {
    // the forward tiles of the workgroups with id % 8 == x: ids [t0, t1) after pyz_xcd_remap, i.e. row blocks from t0 / tiles_n
    const int x = bid & 7, q = g.fwd_tiles >> 3, r = g.fwd_tiles & 7;
    const int t0 = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q, t1 = t0 + (x < r ? q + 1 : q);
    // rows whose first tile lies in [t0, t1)
    const int b0 = (t0 + g.fwd_tiles_n - 1) / g.fwd_tiles_n, b1 = (t1 + g.fwd_tiles_n - 1) / g.fwd_tiles_n;
    const int r0 = min(32 * b0, nb), r1 = x == 7 ? nb : min(32 * b1, nb);
    // the workers with this residue: ids first, first + 8, ... (first = the smallest id >= bid - 8 j with id % 8 == x)
    const int id0 = bid - j;                       // id of worker 0
    const int first = id0 + ((x - (id0 & 7)) & 7); // first worker id with residue x
    const int mine = (bid - first) >> 3, all = (id0 + cnt - 1 - first) / 8 + 1;
    const int per = (r1 - r0 + all - 1) / all;
    ra = r0 + mine * per;
    rb = min(ra + per, r1);
  } else {
    const int per = (nb + cnt - 1) / cnt;
    ra = j * per;
    rb = min(ra + per, nb);
  }
  if (FRAG) pyz_copy_rows_frag(g, idx, ra, rb, nb);
  else pyz_copy_rows(g, idx, ra, rb);
}

// the first batch of a run (nobody ran before it): the same copy as a launch of its own
__global__ void k_prep_batch(PrepArgs g, const StepCtl *ctl) {
  pyz_prep_rows(g, g.row_idx + ctl->row_off, ctl->batch, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.x);
}
__global__ void k_prep_batch_frag(PrepArgs g, const StepCtl *ctl) {   // ... as the two images
  pyz_prep_rows<true>(g, g.row_idx + ctl->row_off, ctl->batch, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.x);
}

// short runs (the tables travel as kernel arguments): k_set_ctl_tabs and k_prep_batch as ONE launch in front of the
// first step -- block 0 writes the tables and the first step's scalars, every block copies its share of the first batch
// (row offset and batch size of that step come as arguments: nothing here reads what block 0 writes)
__global__ void k_run_start(StepCtl *ctl, InlineTabs t, int32_t *tab_bs, float *tab_lr, long long n, long long row_off,
                            int slot0, PrepArgs g) {
  if (blockIdx.x == 0) {
    const int e = threadIdx.x;
    if (e < t.n) {
      tab_bs[e] = t.bs[e];
      tab_lr[e] = t.lr[e];
    }
    if (e == 0) {
      ctl->batch = t.bs[0];
      ctl->lr = t.lr[0];
      ctl->n = n;
      ctl->row_off = row_off;
      ctl->i = 0;
      ctl->slot0 = slot0;
      ctl->n_run = t.n - 1;
    }
  }
  pyz_prep_rows(g, g.row_idx + row_off, t.bs[0], (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.x);
}

// k_run_start of a run that keeps its batches as images (a kernel of its own: k_run_start stays what it was)
__global__ void k_run_start_frag(StepCtl *ctl, InlineTabs t, int32_t *tab_bs, float *tab_lr, long long n, long long row_off,
                                 int slot0, PrepArgs g) {
  if (blockIdx.x == 0) {
    const int e = threadIdx.x;
    if (e < t.n) {
      tab_bs[e] = t.bs[e];
      tab_lr[e] = t.lr[e];
    }
    if (e == 0) {
      ctl->batch = t.bs[0];
      ctl->lr = t.lr[0];
      ctl->n = n;
      ctl->row_off = row_off;
      ctl->i = 0;
      ctl->slot0 = slot0;
      ctl->n_run = t.n - 1;
    }
  }
  pyz_prep_rows<true>(g, g.row_idx + row_off, t.bs[0], (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.x);
}

// k_run_start with the bias-correction table of a device-resident ADAM / VADAM run (k_set_ctl_tabs_bc)
__global__ void k_run_start_bc(StepCtl *ctl, InlineTabs t, InlineBc b, int32_t *tab_bs, float *tab_lr, float2 *tab_bc,
                               long long n, long long row_off, int slot0, PrepArgs g) {
  if (blockIdx.x == 0) {
    const int e = threadIdx.x;
    if (e < t.n) {
      tab_bs[e] = t.bs[e];
      tab_lr[e] = t.lr[e];
      tab_bc[e] = b.bc[e];
    }
    if (e == 0) {
      ctl->batch = t.bs[0];
      ctl->lr = t.lr[0];
      ctl->n = n;
      ctl->row_off = row_off;
      ctl->i = 0;
      ctl->slot0 = slot0;
      ctl->n_run = t.n - 1;
    }
  }
  pyz_prep_rows(g, g.row_idx + row_off, t.bs[0], (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.x);
}

// ---------------------------------------------------------------- all weight gradients + update
struct WgradLayer {
  const float *in;            // layer input: data x (layer 0) or act[l-1]
  long long in_pstride;
  const float *delta;         // (P, max_batch, N)
  long long delta_pstride;
  long long w_off;
  int lda, K, N;
  int tile0;                  // first tile of this layer in the launch
  int gather;                 // rows of `in` go through row_idx (layer 0)
};

#define PYZ_UPD_NONE 0  // write [dW; db] to grad
#define PYZ_UPD_SGD 1   // SGD.py:66-69
#define PYZ_UPD_SGLD 2  // SGLD.py:64-93
#define PYZ_UPD_BBB 3   // BBB.py:152-201 (theta = mu, mean = rho, sq_mean = the sampled w; read only)
#define PYZ_UPD_SWAG 4  // SWAG.py:61-92 (SGD update; gated moments; one deviation row)

// (Field order: what a tile workgroup of k_wgrad_all reads in front of its first operand load comes first -- 136 bytes,
// asked for in one trip -- and the layer it then picks is ONE 64-byte entry of lay[], which starts on a multiple of 64
// (the duties' fields fill the gap); see DenseArgs.  With the layers in front, those fields lay 1 KB into the segment and
// were fetched where each was first used.)
struct WgradArgs {
  int tiles;                  // tiles of all layers; the launch has one more workgroup, for the step duties
  int L;
  int mode;
  int wt;                     // write-through stores for the updated state (pyz_st)
  const StepCtl *ctl;
  const int32_t *row_idx;
  float *theta, *mean, *sq_mean;
  const float *unit_noise;    // SGLD: injected N(0,1); BBB: injected eps
  uint64_t seed;
  int tile0[PYZ_MAX_LAYERS];  // lay[l].tile0 again (INT_MAX past L): a tile finds its layer by comparing with all of them at once
  // duties of workgroup 0 at the end of the step: loss and the next step's scalars
  const double *part;
  int nblk;
  int loss_indexed;
  float *loss;
  StepCtl *next;
  const int32_t *tab_bs;
  const float *tab_lr;
  int *nonfinite;             // device counter of steps with a NaN / Inf loss (may be nullptr)
  WgradLayer lay[PYZ_MAX_LAYERS];
  float *grad;                // mode NONE: (P, D)
  long long grad_pstride;
  // SWAG only: dev_row = the (D) row of the deviation matrix that receives theta - mean, or nullptr
  float *dev_row;
  int swag_update;            // moments / deviation updated at this step (n % frequency == 0)
  // chained SWAG runs (pyz_swag_run): both follow from the step count n -- update when n % swag_freq == 0, into
  // row min(ceil(n / swag_freq), swag_k - 1) of the (swag_k, dev_stride) deviation matrix dev_base
  int swag_freq, swag_k;
  float *dev_base;
  long long dev_stride;
  // BBB only
  float alpha, prior_mean, prior_rho, bbb_lr;
  const float *pm_vec, *pr_vec;
  uint32_t bbb_step;
  int bbb_chained;            // device-resident run: learning rate and step count come from StepCtl, cost goes to slot (slot0 + i)
  const double *part_kl;
  int nblk_kl;
  float *cost;
  // chained BBB runs, sampling fused: the epilogue also draws the NEXT step's weights from the mu / rho it just wrote
  // (w_next, Philox step n + 1 -- k_bbb_sample's arithmetic) and leaves that step's log q - log p partial of its tile in
  // part_kl_next[workgroup]; nullptr = the step's own k_bbb_sample launch does both
  float *w_next;
  double *part_kl_next;
  long long row_stride;       // (duties: the row-table stride between two steps)
  float *ploss;               // particle-batched gradient passes: loss[p] = (sum of particle p's row partials) / batch
  PrepArgs prep;             // chained runs: the workgroups past the duties workgroup assemble the NEXT step's batch
};

static_assert(offsetof(WgradArgs, lay) % 64 == 0 && sizeof(WgradLayer) == 64, "a layer's entry is one 64-byte line");

// ---------------------------------------------------------------- the optimizer updates (shared by the
// epilogue of k_wgrad_all; kept apart from the tile code so that every mode is one readable block)
struct PyzUpdOut {
  float th, mu, sq, dev;
  bool wr_mu, wr_sq, wr_dev;
  float *dev_row;  // SWAG: the deviation row written at this step
};

// gv = d loss / d parameter e; th0 / mu0 / sq0 / zz = the state read before (see the modes above)
__device__ __forceinline__ PyzUpdOut pyz_update_math(const WgradArgs &g, const int mode, const long long e, const float gv,
                                                     const float th0, const float mu0, const float sq0, const float zz,
                                                     const float lr, const long long nstep) {
  PyzUpdOut o;
  o.th = o.mu = o.sq = o.dev = 0.0f;
  o.wr_mu = o.wr_sq = o.wr_dev = false;
  o.dev_row = nullptr;
  // The roundings of the SGD / SWAG / SGLD arms are written out (fmaf = one rounding; everything else in these arms rounds
  // per operation: contraction is off).  They are what k_wgrad_all<16> compiled to while these arms stood in one body with
  // a run-time mode -- there the products mu0 * fn and sq0 * fn were shared by the SWAG and the SGLD arm in front of the
  // branch, out of reach of the sums that might have absorbed them.  Left to the compiler, which of the sums becomes an
  // fma changes with the instantiation and with the code around the call ("The serial head and tail").
  if (mode == PYZ_UPD_SGD) {
    o.th = __builtin_fmaf(-lr, gv, th0);
  } else if (mode == PYZ_UPD_SWAG) {
#pragma clang fp contract(off)
    const float th = __builtin_fmaf(-lr, gv, th0);
    o.th = th;
    const bool upd = g.swag_freq > 0 ? (nstep % g.swag_freq == 0) : (g.swag_update != 0);
    if (upd) {
      const float fn = (float)nstep, fn1 = fn + 1.0f;
      o.mu = (mu0 * fn + th) / fn1;
      o.sq = __builtin_fmaf(th, th, sq0 * fn) / fn1;
      o.dev = th - o.mu;
      o.wr_mu = o.wr_sq = true;
      // columns are appended until there are k; afterwards the LAST one is replaced (SWAG.py:85-89, as written)
      o.dev_row = g.swag_freq > 0
                      ? g.dev_base + min((nstep + g.swag_freq - 1) / g.swag_freq, (long long)g.swag_k - 1) * g.dev_stride
                      : g.dev_row;
      o.wr_dev = o.dev_row != nullptr;
    }
  } else if (mode == PYZ_UPD_BBB) {
    // (Deliberately NOT written out like the arms above: which of this arm's thirty-odd operations fuse is the compiler's
    //  choice, it differed between the instantiations before, and it moves in the last bits when the code around the call
    //  changes -- DESIGN 5, "The serial head and tail".  Pin it here when that matters.)
    // th0 = mu, mu0 = rho, sq0 = the sampled w, zz = eps, gv = d loss / d w   (k_bbb_update's arithmetic)
    const float pmean = g.pm_vec ? g.pm_vec[e] : g.prior_mean;
    const float sp = pyz_softplus(g.pr_vec ? g.pr_vec[e] : g.prior_rho), isp2 = 1.0f / (sp * sp);
    const float mu = th0, rho = mu0, wv = sq0;
    const float sg = pyz_softplus(rho), sig = pyz_sigmoid(rho);
    const float d = wv - mu, is2 = 1.0f / (sg * sg);
    const float g_mu = g.alpha * d * is2;
    const float g_rho = g.alpha * (-1.0f / sg + d * d * is2 / sg) * sig;
    const float g_w = gv + g.alpha * (-d * is2 + (wv - pmean) * isp2);
    const float blr = g.bbb_chained ? lr : g.bbb_lr;
    o.th = mu - blr * (g_mu + g_w);
    o.mu = rho - blr * (zz * sig * g_w + g_rho);
    o.wr_mu = true;
  } else if (mode == PYZ_UPD_SGLD) {
#pragma clang fp contract(off)
    const float fn = (float)nstep, fn1 = fn + 1.0f;
    const float gn = __builtin_fmaf(lr, zz, gv);      // the gradient plus the noise lr * zz
    const float th = __builtin_fmaf(-lr, gn, th0);
    o.th = th;
    o.mu = (mu0 * fn + th) / fn1;
    o.sq = __builtin_fmaf(th, th, sq0 * fn) / fn1;
    o.wr_mu = o.wr_sq = true;
  }
  return o;
}

__device__ __forceinline__ void pyz_update_store(const WgradArgs &g, const int mode, const long long e, const int p,
                                                 const float gv, const PyzUpdOut &o) {
  if (mode == PYZ_UPD_NONE) {
    g.grad[p * g.grad_pstride + e] = gv;
    return;
  }
  pyz_st(g.theta + e, o.th, g.wt);
  if (o.wr_mu) pyz_st(g.mean + e, o.mu, g.wt);
  if (o.wr_sq) pyz_st(g.sq_mean + e, o.sq, g.wt);
  if (o.wr_dev) o.dev_row[e] = o.dev;
}

// duties of one spare wave per step that do not depend on the gradient: the loss of this step
// (partials written by k_head), BBB's cost, and the next step's scalars
__device__ __forceinline__ void pyz_step_duties(const WgradArgs &g, const int l) {
  const int batch = g.ctl->batch;
  if (g.loss) {
    const double v = pyz_sum_partials(g.part, g.nblk);
    if (l == 0) {
      float *lo = g.loss + (g.loss_indexed ? g.ctl->slot0 + g.ctl->i : 0);
      lo[0] = (float)(v / (double)batch);
      pyz_note_loss(g.nonfinite, lo[0]);
      if (g.next) pyz_prepare_next(g.ctl, g.next, g.tab_bs, g.tab_lr, g.row_stride);
    }
  }
  if (g.mode == PYZ_UPD_BBB) {   // cost = loss + alpha (log q - log p)
    const double v = pyz_sum_partials(g.part, g.nblk), k = pyz_sum_partials(g.part_kl, g.nblk_kl);
    if (l == 0) {
      const float loss = (float)(v / (double)batch), kl = (float)k;
      float *co = g.cost + (g.bbb_chained ? 4 * (g.ctl->slot0 + g.ctl->i) : 0);
      co[0] = loss + g.alpha * kl;
      pyz_note_loss(g.nonfinite, co[0]);
      co[1] = loss;
      co[2] = kl;
      if (g.bbb_chained && g.next) pyz_prepare_next(g.ctl, g.next, g.tab_bs, g.tab_lr, g.row_stride);
    }
  }
}

// contiguous (no gather) reduction over the batch rows, software pipelined.  Operands come through
// buffer descriptors built from wave-uniform bases: a step's address is a scalar row offset
// (soffset) plus a per-lane constant (voffset), so the loop spends no vector ALU on addressing.
// Requires batch * row bytes < 2^31 (checked when the plan is created).

template <class H>
__device__ __forceinline__ void pyz_wgrad_accumulate(f32x16 &acc, const float *abase, const int ic, const float *dbase,
                                                     const int n, const int lda, const int N, const int batch, int s,
                                                     const int se, const int h, const bool is_w, const bool is_b, H hook) {
  const float bconst = is_b ? 1.0f : 0.0f;
  const unsigned a_lane = ((unsigned)h * (unsigned)lda + (unsigned)ic) * 4u;
  const unsigned d_lane = ((unsigned)h * (unsigned)N + (unsigned)n) * 4u;
  const unsigned a_row2 = 8u * (unsigned)lda, d_row2 = 8u * (unsigned)N;  // bytes per MFMA step (two rows)
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(abase), 0, (int)((unsigned)batch * (unsigned)lda * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rd =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(dbase), 0, (int)((unsigned)batch * (unsigned)N * 4u), 0x00020000);
  // only whole steps here: the scalar offset is not range checked, so the odd last row is peeled
  const int full = batch >> 1;
  pyz_steps1_all(
      s, min(se, full), acc,
      [&](int st, float &a, float &d) {
        a = pyz_buf_load(ra, a_lane, (unsigned)PYZ_HOT(st, batch) * a_row2);
        d = pyz_buf_load(rd, d_lane, (unsigned)PYZ_HOT(st, batch) * d_row2);
      },
      [&](int, float &a, float &) { a = is_w ? a : bconst; }, hook);
  if (se > full) {  // this wave owns the odd last row: the second reduction slot of its MFMA stays empty
    const int b = batch - 1;
    float a = abase[(size_t)b * lda + ic], d = dbase[(size_t)b * N + n];
    a = h == 0 ? (is_w ? a : bconst) : 0.0f;
    d = h == 0 ? d : 0.0f;
    acc = pyz_mfma(a, d, acc);
  }
}

// pyz_wgrad_accumulate with layer 0's A operand out of the weight-gradient image of the batch (PrepArgs): ablk = this lane's
// piece of row group 0 in the tile's column block, row group g 256 floats further.  One float4 per lane carries the A values
// of the steps 4 g .. 4 g + 3, delta stays one dword per step.  The wave's steps [s, se) run in ascending order exactly as
// above: a group at either end of the range that the wave owns only in part is loaded whole, and the steps outside the range
// are skipped (uniform), not multiplied by zero.
template <class H>
__device__ __forceinline__ void pyz_wgrad_accumulate_frag(f32x16 &acc, const float *ablk, const float *dbase, const int n,
                                                          const int N, const int batch, const int s, const int se,
                                                          const int h, const bool is_w, const bool is_b, H hook) {
  const float bconst = is_b ? 1.0f : 0.0f;
  const unsigned d_lane = ((unsigned)h * (unsigned)N + (unsigned)n) * 4u;
  const unsigned d_row2 = 8u * (unsigned)N;  // bytes per MFMA step (two rows)
  const __amdgpu_buffer_rsrc_t rd =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(dbase), 0, (int)((unsigned)batch * (unsigned)N * 4u), 0x00020000);
  const int full = batch >> 1, sf = min(se, full);   // only whole steps here; the odd last row is peeled (see above)
  const int cb = s >> 2, ce = s < sf ? (sf + 3) >> 2 : cb;
  const int dlast = max(full - 1, 0);                // (the scalar offset is not range checked: no step past the last whole one)
  pyz_pipe4x<2>(
      cb, ce,
      [&](int c, float4 &a4, float4 &d4) {
        const int cc = PYZ_HOT(c, batch);
        a4 = *reinterpret_cast<const float4 *>(ablk + 256 * cc);
        const unsigned s0 = (unsigned)min(4 * cc, dlast), s1 = (unsigned)min(4 * cc + 1, dlast);
        const unsigned s2 = (unsigned)min(4 * cc + 2, dlast), s3 = (unsigned)min(4 * cc + 3, dlast);
        d4 = make_float4(pyz_buf_load(rd, d_lane, s0 * d_row2), pyz_buf_load(rd, d_lane, s1 * d_row2),
                         pyz_buf_load(rd, d_lane, s2 * d_row2), pyz_buf_load(rd, d_lane, s3 * d_row2));
      },
      [&](int c, float4 &a4, float4 &d4) {
        const int st = 4 * c;
        if (st >= s && st < sf) acc = pyz_mfma(is_w ? a4.x : bconst, d4.x, acc);
        if (st + 1 >= s && st + 1 < sf) acc = pyz_mfma(is_w ? a4.y : bconst, d4.y, acc);
        if (st + 2 >= s && st + 2 < sf) acc = pyz_mfma(is_w ? a4.z : bconst, d4.z, acc);
        if (st + 3 >= s && st + 3 < sf) acc = pyz_mfma(is_w ? a4.w : bconst, d4.w, acc);
      },
      hook);
  if (se > full) {  // this wave owns the odd last row (step `full`, h = 0): the second reduction slot of its MFMA stays empty
    const int b = batch - 1;
    float a = ablk[256 * (full >> 2) + (full & 3)], d = dbase[(size_t)b * N + n];
    a = h == 0 ? (is_w ? a : bconst) : 0.0f;
    d = h == 0 ? d : 0.0f;
    acc = pyz_mfma(a, d, acc);
  }
}

// One tile of k_wgrad_all, MODE (the optimizer update) a compile-time constant: the kernel branches once on g.mode, so the
// prefetch hook and the epilogue of an SGLD step hold no other mode's instructions, registers or branches (as one body
// with a run-time mode, BBB's fused sampling -- softplus, logs, the log q - log p reduction -- and SWAG's gated moments lay
// between the SGLD instructions).
// FRAG: layer 0's entry describes the weight-gradient image of the batch (in = the image, lda = its rows, 8 G).
template <int S, bool PLAIN, int MODE, bool FRAG = false>
__device__ __forceinline__ void pyz_wgrad_tile(const WgradArgs &g, float *red) {
  constexpr int EPT = 16 / S;  // tile elements per thread in the epilogue
  const int w = pyz_wave_id(), l = threadIdx.x & 63;
  const int r = l & 31, h = l >> 5;
  const int tile = pyz_xcd_remap(blockIdx.x, g.tiles);
  // the tile's layer: tile0[] is ascending (INT_MAX past the last layer), all sixteen arrived with the first arguments --
  // a count of compares, not a walk with one dependent load per layer
  int li = 0;
#pragma unroll
  for (int j = 1; j < PYZ_MAX_LAYERS; ++j) li += tile >= g.tile0[j] ? 1 : 0;
  li = __builtin_amdgcn_readfirstlane(li);   // (an index, then one address: else the sum is carried out on sixteen address candidates)
  const WgradLayer &ly = g.lay[li];
  // the step scalars (written by another kernel: vector loads) and the layer's entry travel together: one wait each
  const PyzCtlHot ctl_raw = pyz_ctl_request(g.ctl);
  asm volatile("; the layer in one trip" ::"s"(ly.in), "s"(ly.in_pstride), "s"(ly.delta), "s"(ly.delta_pstride), "s"(ly.w_off),
               "s"(ly.lda), "s"(ly.K), "s"(ly.N), "s"(ly.tile0), "s"(ly.gather));
  const PyzCtlHot ctl = pyz_ctl_arrived(ctl_raw);
  const int batch = ctl.batch;
  const int K = ly.K, N = ly.N;
  const int tiles_n = (N + 31) >> 5;
  const int t = tile - ly.tile0;
  const int i0 = (t / tiles_n) * 32, n0 = (t % tiles_n) * 32;
  const int p = blockIdx.y;
  const long long w_off = ly.w_off;
  constexpr int mode = PLAIN ? PYZ_UPD_NONE : MODE;
  const long long nstep = ctl.n;
  const float lr = ctl.lr;

  // -- epilogue operands of this thread's elements and the Philox noise: needed only after the
  //    reduction, so they are fetched / generated right behind the first group of operand loads
  //    (the hook of the pipelined loop) and their latency hides behind the loads and MFMAs
  long long ee[EPT];
  bool ev[EPT];
  float th0[PLAIN ? 1 : EPT], mu0[PLAIN ? 1 : EPT], sq0[PLAIN ? 1 : EPT], zz[PLAIN ? 1 : EPT];
  float zg[PLAIN ? 1 : EPT];   // generated noise: its own registers (writing a register a load may still be filling waits for EVERY load in flight)
  float zn[PLAIN ? 1 : EPT];   // BBB with fused sampling: the next step's eps
  const bool fuse_next = !PLAIN && mode == PYZ_UPD_BBB && g.w_next != nullptr;
  auto prefetch = [&]() {
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      int ro, co;
      if (S == 1) {
        ro = (q & 3) + 8 * (q >> 2) + 4 * h;
        co = r;
      } else {
        const int e = threadIdx.x + q * 64 * S;
        ro = e >> 5;
        co = e & 31;
      }
      const int ii = i0 + ro, nn = n0 + co;
      ev[q] = ii <= K && nn < N;
      ee[q] = w_off + (long long)min(ii, K) * N + min(nn, N - 1);
      if (PLAIN) continue;
      th0[q] = mu0[q] = sq0[q] = zz[q] = zg[q] = 0.0f;
      if (mode != PYZ_UPD_NONE) th0[q] = g.theta[ee[q]];
      if (mode == PYZ_UPD_SGLD || mode == PYZ_UPD_BBB || mode == PYZ_UPD_SWAG) {
        mu0[q] = g.mean[ee[q]];
        sq0[q] = g.sq_mean[ee[q]];
        if (g.unit_noise && mode != PYZ_UPD_SWAG) zz[q] = g.unit_noise[ee[q]];
      }
    }
    if (!PLAIN && (mode == PYZ_UPD_SGLD || mode == PYZ_UPD_BBB) && !g.unit_noise) {
#pragma unroll
      for (int q = 0; q < EPT; ++q) {
        zg[q] = mode == PYZ_UPD_SGLD ? pyz_normal1(g.seed, PYZ_STREAM_SGLD, (uint32_t)nstep, (uint64_t)ee[q])
                                     : pyz_normal1(g.seed, PYZ_STREAM_BBB, g.bbb_chained ? (uint32_t)nstep : g.bbb_step, (uint64_t)ee[q]);
      }
    }
    if (!PLAIN && fuse_next) {
#pragma unroll
      for (int q = 0; q < EPT; ++q) zn[q] = pyz_normal1(g.seed, PYZ_STREAM_BBB, (uint32_t)(nstep + 1), (uint64_t)ee[q]);
    }
  };

  const int i = i0 + r, n = min(n0 + r, N - 1);
  const int ic = min(i, K - 1);
  const bool is_w = i < K, is_b = i == K;
  const float *ap = ly.in + p * ly.in_pstride + ic;
  const float *dp = ly.delta + p * ly.delta_pstride + n;
  const int32_t *idx = (ly.gather && g.row_idx) ? g.row_idx + ctl.row_off : nullptr;
  f32x16 acc = {0};
  const int steps = (batch + 1) >> 1;
  int s = (steps * w) / S;
  const int se = (steps * (w + 1)) / S;
  PYZ_STAMP(2, 1);
  if (FRAG && li == 0) {   // (uniform)
    // the tile's column block of the image; a tile that holds only the bias row (K % 32 == 0) reads the last block and
    // uses none of it
    const int kb = min(i0, K - 1) >> 5, G = ly.lda >> 3;
    pyz_wgrad_accumulate_frag(acc, ly.in + ((long long)kb * G * 64 + l) * 4, ly.delta + p * ly.delta_pstride, n, N, batch, s,
                              se, h, is_w, is_b, prefetch);
  } else if (idx) {
    prefetch();
    // gathered rows: the 64 row indices of a 32-step chunk come from ONE coalesced load (lane j
    // holds the index of batch row 2*s0 + j) and reach the step that needs them by a lane
    // permute, so the pipelined operand loads never wait on an index load
    for (int s0 = s; s0 < se; s0 += 32) {
      const int idxv = idx[min(2 * s0 + l, batch - 1)];
      const int lda = ly.lda;
      pyz_steps1_all(
          s0, min(s0 + 32, se), acc,
          [&](int st, float &a, float &d) {
            const int bc = PYZ_HOT(min(2 * st + h, batch - 1), batch);
            const long long row = PYZ_HOT(__shfl(idxv, 2 * (st - s0) + h, 64), batch);
            a = ap[row * lda];
            d = dp[(long long)bc * N];
          },
          [&](int st, float &a, float &d) {
            const bool vb = 2 * st + h < batch;
            a = vb ? (is_w ? a : (is_b ? 1.0f : 0.0f)) : 0.0f;
            d = vb ? d : 0.0f;
          });
    }
  } else {
    pyz_wgrad_accumulate(acc, ly.in + p * ly.in_pstride, ic, ly.delta + p * ly.delta_pstride, n, ly.lda, N, batch, s, se, h,
                         is_w, is_b, prefetch);
  }
  PYZ_STAMP(2, 2);
  float gv[EPT];
  if (S == 1) {
#pragma unroll
    for (int q = 0; q < EPT; ++q) gv[q] = acc[q];
  } else {
    float *my = red + w * 1024;
#pragma unroll
    for (int q = 0; q < 16; ++q) my[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = acc[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = threadIdx.x + q * 64 * S;
      float v = red[e];
#pragma unroll
      for (int ww = 1; ww < S; ++ww) v += red[ww * 1024 + e];
      gv[q] = v;
    }
  }
  PYZ_STAMP(2, 4);
  double klp = 0.0;
  float sp_s = 1.0f, lsp_s = 0.0f;
  if (!PLAIN && fuse_next) {
    sp_s = pyz_softplus(g.prior_rho);
    lsp_s = logf(sp_s);
  }
#pragma unroll
  for (int q = 0; q < EPT; ++q) {
    if (!ev[q]) continue;
    if (PLAIN) {
      pyz_st(g.grad + p * g.grad_pstride + ee[q], gv[q], g.wt);
      continue;
    }
    const PyzUpdOut o = pyz_update_math(g, mode, ee[q], gv[q], th0[q], mu0[q], sq0[q],
                                        PLAIN ? 0.0f : (g.unit_noise ? zz[q] : zg[q]), lr, nstep);
    pyz_update_store(g, mode, ee[q], p, gv[q], o);
    if (fuse_next) {   // k_bbb_sample's element, from the mu (o.th) and rho (o.mu) of this update
      const long long e = ee[q];
      const float pmean = g.pm_vec ? g.pm_vec[e] : g.prior_mean;
      float sp = sp_s, lsp = lsp_s;
      if (g.pr_vec) {
        sp = pyz_softplus(g.pr_vec[e]);
        lsp = logf(sp);
      }
      const float mu = o.th, sg = pyz_softplus(o.mu);
      const float wn = zn[q] * sg + mu;
      pyz_st(g.w_next + e, wn, g.wt);
      const float a = (wn - mu) / sg, b = (wn - pmean) / sp;
      const float lq = -0.5f * a * a - logf(sg) - PYZ_LOG_SQRT_2PI;
      const float lp = -0.5f * b * b - lsp - PYZ_LOG_SQRT_2PI;
      klp += (double)lq - (double)lp;
    }
  }
  if (!PLAIN && fuse_next) {   // (uniform over the launch) this tile's share of the next step's log q - log p
    double tot = pyz_wave_sum(klp);
    if (S > 1) {
      double *sm = reinterpret_cast<double *>(red);
      __syncthreads();   // every wave is done reading the tile partials in `red`
      if (l == 0) sm[w] = tot;
      __syncthreads();
      tot = 0.0;
      if (threadIdx.x == 0)
        for (int ww = 0; ww < S; ++ww) tot += sm[ww];
    }
    if (threadIdx.x == 0) g.part_kl_next[blockIdx.x] = tot;
  }
  PYZ_STAMP(2, 3);
}

// S = waves per workgroup (compile time: the epilogue prefetches 16/S elements per thread).
// PLAIN: the launch only writes gradients (g.mode == PYZ_UPD_NONE: particle-batched passes of SVGD / HMC, loss_grad):
// no optimizer state is fetched, so the four prefetch arrays of the epilogue do not exist -- for S = 1 that is 64
// registers per lane, i.e. the difference between two and four resident waves per SIMD.
template <int S, bool PLAIN = false>
__global__ void __launch_bounds__(64 * S) k_wgrad_all(WgradArgs g) {
  extern __shared__ float red[];
  PYZ_STAMP(2, 0);
  const int w = pyz_wave_id(), l = threadIdx.x & 63;
  // what a tile workgroup needs in front of its first operand load, in one trip (see WgradArgs)
  asm volatile("; arguments in one trip" ::"s"(g.tiles), "s"(g.mode), "s"(g.ctl), "s"(g.row_idx), "s"(g.tile0[1]),
               "s"(g.tile0[2]), "s"(g.tile0[3]), "s"(g.tile0[4]), "s"(g.tile0[5]), "s"(g.tile0[6]), "s"(g.tile0[7]),
               "s"(g.tile0[8]), "s"(g.tile0[9]), "s"(g.tile0[10]), "s"(g.tile0[11]), "s"(g.tile0[12]), "s"(g.tile0[13]),
               "s"(g.tile0[14]), "s"(g.tile0[15]));
  // workgroup `tiles` (the last id) owns no tile: its first wave does the duties of the step that do
  // not depend on the gradient, off the critical path of the tile workgroups
  if (blockIdx.x >= (unsigned)g.tiles) {  // (without a batch to prepare, ids past `tiles` + 1 only pad the launch)
    if (blockIdx.x == (unsigned)g.tiles && blockIdx.y == 0 && w == 0) pyz_step_duties(g, l);
    if (blockIdx.x == (unsigned)g.tiles && w == 0 && g.ploss) {   // every particle's spare workgroup: its loss (k_loss_finalize)
      const double tot = pyz_sum_partials(g.part + (long long)blockIdx.y * g.nblk, g.nblk);
      if (l == 0) {
        g.ploss[blockIdx.y] = (float)(tot / (double)g.ctl->batch);
        pyz_note_loss(g.nonfinite, g.ploss[blockIdx.y]);
      }
    }
    if (!PLAIN && blockIdx.x > (unsigned)g.tiles && blockIdx.y == 0 && g.prep.src) {
      const int i2 = g.ctl->i + 1;
      if (i2 < g.ctl->n_run)
        pyz_prep_rows(g.prep, g.prep.row_idx + g.ctl->row_off + g.prep.row_stride, g.prep.tab_bs[i2],
                      (int)blockIdx.x - g.tiles - 1, (int)gridDim.x - g.tiles - 1, (int)blockIdx.x);
      PYZ_STAMP(2, 3);
    }
    return;
  }
  // (uniform) one instruction stream per update mode
  if constexpr (PLAIN) {
    pyz_wgrad_tile<S, true, PYZ_UPD_NONE>(g, red);
  } else {
    switch (g.mode) {
      case PYZ_UPD_SGLD: pyz_wgrad_tile<S, false, PYZ_UPD_SGLD>(g, red); break;
      case PYZ_UPD_SGD: pyz_wgrad_tile<S, false, PYZ_UPD_SGD>(g, red); break;
      case PYZ_UPD_SWAG: pyz_wgrad_tile<S, false, PYZ_UPD_SWAG>(g, red); break;
      case PYZ_UPD_BBB: pyz_wgrad_tile<S, false, PYZ_UPD_BBB>(g, red); break;
      default: pyz_wgrad_tile<S, false, PYZ_UPD_NONE>(g, red); break;
    }
  }
}

// k_wgrad_all of a run whose batches stand as images: layer 0's tiles read this step's weight-gradient image
// (pyz_wgrad_tile<.., true>) and the workers leave the next batch as images.  One chain, an updating mode; a kernel of its own,
// so that every k_wgrad_all<S> stays what it was.
template <int S>
__global__ void __launch_bounds__(64 * S) k_wgrad_all_frag(WgradArgs g) {
  extern __shared__ float red[];
  PYZ_STAMP(2, 0);
  const int w = pyz_wave_id(), l = threadIdx.x & 63;
  asm volatile("; arguments in one trip" ::"s"(g.tiles), "s"(g.mode), "s"(g.ctl), "s"(g.row_idx), "s"(g.tile0[1]),
               "s"(g.tile0[2]), "s"(g.tile0[3]), "s"(g.tile0[4]), "s"(g.tile0[5]), "s"(g.tile0[6]), "s"(g.tile0[7]),
               "s"(g.tile0[8]), "s"(g.tile0[9]), "s"(g.tile0[10]), "s"(g.tile0[11]), "s"(g.tile0[12]), "s"(g.tile0[13]),
               "s"(g.tile0[14]), "s"(g.tile0[15]));
  if (blockIdx.x >= (unsigned)g.tiles) {
    if (blockIdx.x == (unsigned)g.tiles && w == 0) pyz_step_duties(g, l);
    if (blockIdx.x > (unsigned)g.tiles && g.prep.src) {
      const int i2 = g.ctl->i + 1;
      if (i2 < g.ctl->n_run)
        pyz_prep_rows<true>(g.prep, g.prep.row_idx + g.ctl->row_off + g.prep.row_stride, g.prep.tab_bs[i2],
                            (int)blockIdx.x - g.tiles - 1, (int)gridDim.x - g.tiles - 1, (int)blockIdx.x);
      PYZ_STAMP(2, 3);
    }
    return;
  }
  switch (g.mode) {   // (uniform) one instruction stream per update mode
    case PYZ_UPD_SGLD: pyz_wgrad_tile<S, false, PYZ_UPD_SGLD, true>(g, red); break;
    case PYZ_UPD_SGD: pyz_wgrad_tile<S, false, PYZ_UPD_SGD, true>(g, red); break;
    case PYZ_UPD_SWAG: pyz_wgrad_tile<S, false, PYZ_UPD_SWAG, true>(g, red); break;
    case PYZ_UPD_BBB: pyz_wgrad_tile<S, false, PYZ_UPD_BBB, true>(g, red); break;
    default: __builtin_trap();   // no other mode's run assembles images
  }
}

// pyz_wgrad_accumulate with a second chain: acc2 += (a^2) (fb d)^2 from the masked operands of every step (k_wgrad_adam)
template <class H>
__device__ __forceinline__ void pyz_wgrad_accumulate_sq(f32x16 &acc, f32x16 &acc2, const float fb, const float *abase,
                                                        const int ic, const float *dbase, const int n, const int lda,
                                                        const int N, const int batch, int s, const int se, const int h,
                                                        const bool is_w, const bool is_b, H hook) {
  const float bconst = is_b ? 1.0f : 0.0f;
  const unsigned a_lane = ((unsigned)h * (unsigned)lda + (unsigned)ic) * 4u;
  const unsigned d_lane = ((unsigned)h * (unsigned)N + (unsigned)n) * 4u;
  const unsigned a_row2 = 8u * (unsigned)lda, d_row2 = 8u * (unsigned)N;  // bytes per MFMA step (two rows)
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(abase), 0, (int)((unsigned)batch * (unsigned)lda * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rd =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(dbase), 0, (int)((unsigned)batch * (unsigned)N * 4u), 0x00020000);
  // only whole steps here: the scalar offset is not range checked, so the odd last row is peeled
  const int full = batch >> 1;
  pyz_steps1_all(
      s, min(se, full), acc,
      [&](int st, float &a, float &d) {
        a = pyz_buf_load(ra, a_lane, (unsigned)PYZ_HOT(st, batch) * a_row2);
        d = pyz_buf_load(rd, d_lane, (unsigned)PYZ_HOT(st, batch) * d_row2);
      },
      [&](int, float &a, float &d) {
        a = is_w ? a : bconst;
        const float gd = d * fb;
        acc2 = pyz_mfma(a * a, gd * gd, acc2);
      },
      hook);
  if (se > full) {  // this wave owns the odd last row: the second reduction slot of its MFMA stays empty
    const int b = batch - 1;
    float a = abase[(size_t)b * lda + ic], d = dbase[(size_t)b * N + n];
    a = h == 0 ? (is_w ? a : bconst) : 0.0f;
    d = h == 0 ? d : 0.0f;
    const float gd = d * fb;
    acc2 = pyz_mfma(a * a, gd * gd, acc2);
    acc = pyz_mfma(a, d, acc);
  }
}

// ---------------------------------------------------------------- ADAM / VADAM: gradients, their second moment, update
// ADAM.step / VADAM.step need per parameter the batch mean g of the per-example gradients and the batch mean s of their
// squares (the reference squares a (B, D) tape.jacobian: ADAM.py:60-75, VADAM.py:67-96).  For a Dense layer the
// per-example gradient of [W; b] is a_i (x) (B delta_i) -- delta carries the 1/B of the mean loss (k_head) -- so
//     s = (1/B) (A o A)^T ((B Delta) o (B Delta)),
// the reduction over the batch that k_wgrad_all runs for A^T Delta, on squared operands: a second MFMA chain beside the
// first, fed from the registers the operands were loaded into (no Jacobian, no second pass over the activations).
// Scaling: delta is multiplied by B BEFORE it is squared, so the chain sums squares of per-example gradients (what the
// reference squares) and only the final sum is divided by B; squaring delta itself (g^2 / B^2) would send every
// per-example gradient below ~1e-19 * B through the float32 subnormals.  B is the step's batch (ctl->batch: the last batch
// of an epoch is shorter).  The two tiles are combined across waves through the same `red` buffer, one after the other.
// A kernel of its own (not a mode of k_wgrad_all): the SGD / SGLD / SWAG / BBB / PLAIN instantiations are left as they were.
struct AdamArgs {
  WgradArgs w;   // layers, tiles, theta, the duties (loss, nonfinite); mode PYZ_UPD_NONE, grad unused
  float *m, *v;
  AdamScal a;
};

// Device-resident runs (pyz_adam_run / pyz_bsam_run): the chained form of the two kernels takes the step's learning rate
// from StepCtl and ADAM's bias-correction pair from the per-run table at ctl->i, writes the loss at the step's slot,
// prepares the other StepCtl slot, assembles the next step's batch in its spare workgroups (k_wgrad_all's PrepArgs) and --
// `perturb`, while step i + 1 exists -- stores the weight with the perturbation of step i + 1 already applied: that
// perturbation reads only the v and the weight this epilogue holds in registers (VADAM.py:59-65, BSAM.py:63-68), so the
// run has no perturbation launch after its first step.  The last step of a call stores the unperturbed weight.
struct RunChain {
  const float2 *tab_bc;   // ADAM / VADAM: {1 - beta_1^epoch, 1 - beta_2^epoch} per step of the run
  int perturb;            // 0: the run perturbs in a launch of its own (or not at all: ADAM)
  float lam, num_data;    // VADAM's perturbation
};

// duties of the spare workgroup in a chained launch: the loss of step i to loss[stride (slot0 + i) + off], and -- `advance` --
// the next step's scalars
__device__ __forceinline__ void pyz_run_duties(const WgradArgs &g, const int l, const int stride, const int off,
                                               const bool advance) {
  const double v = pyz_sum_partials(g.part, g.nblk);
  if (l == 0) {
    float *lo = g.loss + (long long)stride * (g.ctl->slot0 + g.ctl->i) + off;
    lo[0] = (float)(v / (double)g.ctl->batch);
    pyz_note_loss(g.nonfinite, lo[0]);
    if (advance) pyz_prepare_next(g.ctl, g.next, g.tab_bs, g.tab_lr, g.row_stride);
  }
}

// the workgroups past the duties workgroup of a chained launch: the next step's batch (see k_wgrad_all)
__device__ __forceinline__ void pyz_run_prep(const WgradArgs &g) {
  if (blockIdx.x > (unsigned)g.tiles && g.prep.src) {
    const int i2 = g.ctl->i + 1;
    if (i2 < g.ctl->n_run)
      pyz_prep_rows(g.prep, g.prep.row_idx + g.ctl->row_off + g.prep.row_stride, g.prep.tab_bs[i2],
                    (int)blockIdx.x - g.tiles - 1, (int)gridDim.x - g.tiles - 1, (int)blockIdx.x);
  }
}

struct AdamRunArgs : AdamArgs {
  RunChain c;
};

// CHAIN: the chained form (AdamRunArgs); the eager instantiations k_wgrad_adam<S> contain none of it
template <int S, bool CHAIN = false>
__global__ void __launch_bounds__(64 * S) k_wgrad_adam(std::conditional_t<CHAIN, AdamRunArgs, AdamArgs> A) {
  extern __shared__ float red[];
  const WgradArgs &g = A.w;
  constexpr int EPT = 16 / S;  // tile elements per thread in the epilogue
  const int w = pyz_wave_id(), l = threadIdx.x & 63;
  const int r = l & 31, h = l >> 5;
  if (blockIdx.x >= (unsigned)g.tiles) {  // the duties workgroup: the step's loss and the non-finite count
    if constexpr (CHAIN) {
      if (blockIdx.x == (unsigned)g.tiles && w == 0) pyz_run_duties(g, l, 1, 0, true);
      pyz_run_prep(g);
    } else {
      if (blockIdx.x == (unsigned)g.tiles && w == 0) pyz_step_duties(g, l);
    }
    return;
  }
  const int tile = pyz_xcd_remap(blockIdx.x, g.tiles);
  int li = 0;
  while (li + 1 < g.L && tile >= g.lay[li + 1].tile0) ++li;
  const WgradLayer &ly = g.lay[li];
  const int batch = g.ctl->batch;
  const int K = ly.K, N = ly.N;
  const int tiles_n = (N + 31) >> 5;
  const int t = tile - ly.tile0;
  const int i0 = (t / tiles_n) * 32, n0 = (t % tiles_n) * 32;
  const long long w_off = ly.w_off;

  // the state of this thread's elements, fetched behind the first group of operand loads (see k_wgrad_all)
  long long ee[EPT];
  bool ev[EPT];
  float th0[EPT], m0[EPT], v0[EPT];
  float zn[CHAIN ? EPT : 1];   // chained, perturbing: the next step's eps
  AdamScal sc;                 // chained: the update's scalars with this step's lr, bc1, bc2
  bool perturb_next = false;
  if constexpr (CHAIN) {
    const int si = g.ctl->i;
    const float2 bc = A.c.tab_bc[si];
    sc = A.a;
    sc.lr = g.ctl->lr;
    sc.bc1 = bc.x;
    sc.bc2 = bc.y;
    perturb_next = A.c.perturb && si + 1 < g.ctl->n_run;
  }
  auto prefetch = [&]() {
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      int ro, co;
      if (S == 1) {
        ro = (q & 3) + 8 * (q >> 2) + 4 * h;
        co = r;
      } else {
        const int e = threadIdx.x + q * 64 * S;
        ro = e >> 5;
        co = e & 31;
      }
      const int ii = i0 + ro, nn = n0 + co;
      ev[q] = ii <= K && nn < N;
      ee[q] = w_off + (long long)min(ii, K) * N + min(nn, N - 1);
      th0[q] = g.theta[ee[q]];
      m0[q] = A.m[ee[q]];
      v0[q] = A.v[ee[q]];
    }
    if constexpr (CHAIN) {
      if (perturb_next) {
        const uint32_t n1 = (uint32_t)(g.ctl->n + 1);
#pragma unroll
        for (int q = 0; q < EPT; ++q) zn[q] = pyz_normal1(g.seed, PYZ_STREAM_VADAM, n1, (uint64_t)ee[q]);
      }
    }
  };

  const int i = i0 + r, n = min(n0 + r, N - 1);
  const int ic = min(i, K - 1);
  const bool is_w = i < K, is_b = i == K;
  const float *ap = ly.in + ic;
  const float *dp = ly.delta + n;
  const int32_t *idx = (ly.gather && g.row_idx) ? g.row_idx + g.ctl->row_off : nullptr;
  const float fb = (float)batch;
  f32x16 acc = {0}, acc2 = {0};
  const int steps = (batch + 1) >> 1;
  int s = (steps * w) / S;
  const int se = (steps * (w + 1)) / S;
  if (idx) {
    prefetch();
    for (int s0 = s; s0 < se; s0 += 32) {   // gathered rows: k_wgrad_all's index broadcast
      const int idxv = idx[min(2 * s0 + l, batch - 1)];
      const int lda = ly.lda;
      pyz_steps1_all(
          s0, min(s0 + 32, se), acc,
          [&](int st, float &a, float &d) {
            const int bc = min(2 * st + h, batch - 1);
            const long long row = __shfl(idxv, 2 * (st - s0) + h, 64);
            a = ap[row * lda];
            d = dp[(long long)bc * N];
          },
          [&](int st, float &a, float &d) {
            const bool vb = 2 * st + h < batch;
            a = vb ? (is_w ? a : (is_b ? 1.0f : 0.0f)) : 0.0f;
            d = vb ? d : 0.0f;
            const float gd = d * fb;
            acc2 = pyz_mfma(a * a, gd * gd, acc2);
          });
    }
  } else {
    pyz_wgrad_accumulate_sq(acc, acc2, fb, ly.in, ic, ly.delta, n, ly.lda, N, batch, s, se, h, is_w, is_b, prefetch);
  }
  float gv[EPT], sv[EPT];
  if (S == 1) {
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      gv[q] = acc[q];
      sv[q] = acc2[q];
    }
  } else {
    float *my = red + w * 1024;
#pragma unroll
    for (int q = 0; q < 16; ++q) my[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = acc[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = threadIdx.x + q * 64 * S;
      float v = red[e];
#pragma unroll
      for (int ww = 1; ww < S; ++ww) v += red[ww * 1024 + e];
      gv[q] = v;
    }
    __syncthreads();   // every wave has read the first round
#pragma unroll
    for (int q = 0; q < 16; ++q) my[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = acc2[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = threadIdx.x + q * 64 * S;
      float v = red[e];
#pragma unroll
      for (int ww = 1; ww < S; ++ww) v += red[ww * 1024 + e];
      sv[q] = v;
    }
  }
#pragma unroll
  for (int q = 0; q < EPT; ++q) {
    if (!ev[q]) continue;
    if constexpr (CHAIN) {
      const PyzAdamOut o = pyz_adam_math_pinned(sc, th0[q], m0[q], v0[q], gv[q], sv[q] / fb);
      const float th = perturb_next ? pyz_vadam_perturb_math(A.c.num_data, A.c.lam, o.th, o.v, zn[q]) : o.th;
      pyz_st(g.theta + ee[q], th, g.wt);
      pyz_st(A.m + ee[q], o.m, g.wt);
      pyz_st(A.v + ee[q], o.v, g.wt);
    } else {
      const PyzAdamOut o = pyz_adam_math(A.a, th0[q], m0[q], v0[q], gv[q], sv[q] / fb);
      pyz_st(g.theta + ee[q], o.th, g.wt);
      pyz_st(A.m + ee[q], o.m, g.wt);
      pyz_st(A.v + ee[q], o.v, g.wt);
    }
  }
}


// ---------------------------------------------------------------- BSAM: gradients + ascent, gradients + update
// BSAM.step (BSAM.py:46-119) takes two gradient passes on one batch.  After the first the weights ascend along g1 / v
// and g1 is kept; after the second m, v and the weights are updated from g2 and the kept g1 (pyz_bsam_ascent_math /
// pyz_bsam_math, pyz_kernels.h).  Both are elementwise in the gradient tile a workgroup of k_wgrad_all has just reduced,
// so each pass ends in the epilogue of its weight-gradient launch: k_wgrad_all's tile walk, one MFMA chain, the
// reduction across the S waves through LDS and the duties workgroup (loss, non-finite count), with
//   PHASE 0: reads w, v;         writes g1 (the tile's gradient) and w <- w + rho g1 / v
//   PHASE 1: reads w, m, v, g1;  writes m, v and w
// No launch reads the weights after the head and the data-gradient kernels of its pass, so they are updated in place.
// A kernel of its own (not a mode of k_wgrad_all or k_wgrad_adam): their instantiations are left as they were.
struct BsamArgs {
  WgradArgs w;   // layers, tiles, theta, the duties (loss, nonfinite); mode PYZ_UPD_NONE, grad unused
  float *m, *v, *g1;
  BsamScal a;
};

struct BsamRunArgs : BsamArgs {
  RunChain c;
};

// CHAIN: the chained form (BsamRunArgs); the eager instantiations k_wgrad_bsam<S, PHASE> contain none of it
template <int S, int PHASE, bool CHAIN = false>
__global__ void __launch_bounds__(64 * S) k_wgrad_bsam(std::conditional_t<CHAIN, BsamRunArgs, BsamArgs> A) {
  extern __shared__ float red[];
  const WgradArgs &g = A.w;
  constexpr int EPT = 16 / S;  // tile elements per thread in the epilogue
  const int w = pyz_wave_id(), l = threadIdx.x & 63;
  const int r = l & 31, h = l >> 5;
  if (blockIdx.x >= (unsigned)g.tiles) {  // the duties workgroup: the pass's loss and the non-finite count
    if constexpr (CHAIN) {   // {l1, l2} of step i at 2 (slot0 + i); only the second pass advances the StepCtl
      if (blockIdx.x == (unsigned)g.tiles && w == 0) pyz_run_duties(g, l, 2, PHASE, PHASE == 1);
      if constexpr (PHASE == 1) pyz_run_prep(g);
    } else {
      if (blockIdx.x == (unsigned)g.tiles && w == 0) pyz_step_duties(g, l);
    }
    return;
  }
  const int tile = pyz_xcd_remap(blockIdx.x, g.tiles);
  int li = 0;
  while (li + 1 < g.L && tile >= g.lay[li + 1].tile0) ++li;
  const WgradLayer &ly = g.lay[li];
  const int batch = g.ctl->batch;
  const int K = ly.K, N = ly.N;
  const int tiles_n = (N + 31) >> 5;
  const int t = tile - ly.tile0;
  const int i0 = (t / tiles_n) * 32, n0 = (t % tiles_n) * 32;
  const long long w_off = ly.w_off;

  // the state of this thread's elements, fetched behind the first group of operand loads (see k_wgrad_all)
  long long ee[EPT];
  bool ev[EPT];
  float th0[EPT], v0[EPT], m0[PHASE ? EPT : 1], g10[PHASE ? EPT : 1];
  float zn[(CHAIN && PHASE) ? EPT : 1];   // chained second pass, perturbing: the next step's eps
  BsamScal sc;                            // chained: the step's scalars with its lr
  bool perturb_next = false;
  if constexpr (CHAIN) {
    sc = A.a;
    sc.lr = g.ctl->lr;
    if constexpr (PHASE == 1) perturb_next = A.c.perturb && g.ctl->i + 1 < g.ctl->n_run;
  }
  auto prefetch = [&]() {
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      int ro, co;
      if (S == 1) {
        ro = (q & 3) + 8 * (q >> 2) + 4 * h;
        co = r;
      } else {
        const int e = threadIdx.x + q * 64 * S;
        ro = e >> 5;
        co = e & 31;
      }
      const int ii = i0 + ro, nn = n0 + co;
      ev[q] = ii <= K && nn < N;
      ee[q] = w_off + (long long)min(ii, K) * N + min(nn, N - 1);
      th0[q] = g.theta[ee[q]];
      v0[q] = A.v[ee[q]];
      if constexpr (PHASE == 1) {
        m0[q] = A.m[ee[q]];
        g10[q] = A.g1[ee[q]];
      }
    }
    if constexpr (CHAIN && PHASE == 1) {
      if (perturb_next) {
        const uint32_t n1 = (uint32_t)(g.ctl->n + 1);
#pragma unroll
        for (int q = 0; q < EPT; ++q) zn[q] = pyz_normal1(g.seed, PYZ_STREAM_BSAM, n1, (uint64_t)ee[q]);
      }
    }
  };

  const int i = i0 + r, n = min(n0 + r, N - 1);
  const int ic = min(i, K - 1);
  const bool is_w = i < K, is_b = i == K;
  const float *ap = ly.in + ic;
  const float *dp = ly.delta + n;
  const int32_t *idx = (ly.gather && g.row_idx) ? g.row_idx + g.ctl->row_off : nullptr;
  f32x16 acc = {0};
  const int steps = (batch + 1) >> 1;
  int s = (steps * w) / S;
  const int se = (steps * (w + 1)) / S;
  if (idx) {
    prefetch();
    for (int s0 = s; s0 < se; s0 += 32) {   // gathered rows: k_wgrad_all's index broadcast
      const int idxv = idx[min(2 * s0 + l, batch - 1)];
      const int lda = ly.lda;
      pyz_steps1_all(
          s0, min(s0 + 32, se), acc,
          [&](int st, float &a, float &d) {
            const int bc = PYZ_HOT(min(2 * st + h, batch - 1), batch);
            const long long row = PYZ_HOT(__shfl(idxv, 2 * (st - s0) + h, 64), batch);
            a = ap[row * lda];
            d = dp[(long long)bc * N];
          },
          [&](int st, float &a, float &d) {
            const bool vb = 2 * st + h < batch;
            a = vb ? (is_w ? a : (is_b ? 1.0f : 0.0f)) : 0.0f;
            d = vb ? d : 0.0f;
          });
    }
  } else {
    pyz_wgrad_accumulate(acc, ly.in, ic, ly.delta, n, ly.lda, N, batch, s, se, h, is_w, is_b, prefetch);
  }
  float gv[EPT];
  if (S == 1) {
#pragma unroll
    for (int q = 0; q < EPT; ++q) gv[q] = acc[q];
  } else {
    float *my = red + w * 1024;
#pragma unroll
    for (int q = 0; q < 16; ++q) my[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = acc[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = threadIdx.x + q * 64 * S;
      float v = red[e];
#pragma unroll
      for (int ww = 1; ww < S; ++ww) v += red[ww * 1024 + e];
      gv[q] = v;
    }
  }
#pragma unroll
  for (int q = 0; q < EPT; ++q) {
    if (!ev[q]) continue;
    if constexpr (PHASE == 0) {
      pyz_st(A.g1 + ee[q], gv[q], g.wt);
      pyz_st(g.theta + ee[q], pyz_bsam_ascent_math(A.a, th0[q], v0[q], gv[q]), g.wt);   // (rho: lr plays no part)
    } else if constexpr (CHAIN) {
      const PyzBsamOut o = pyz_bsam_math(sc, th0[q], m0[q], v0[q], gv[q], g10[q]);
      const float th = perturb_next ? pyz_bsam_perturb_math(sc.inv_n, o.th, o.v, zn[q]) : o.th;
      pyz_st(g.theta + ee[q], th, g.wt);
      pyz_st(A.m + ee[q], o.m, g.wt);
      pyz_st(A.v + ee[q], o.v, g.wt);
    } else {
      const PyzBsamOut o = pyz_bsam_math(A.a, th0[q], m0[q], v0[q], gv[q], g10[q]);
      pyz_st(g.theta + ee[q], o.th, g.wt);
      pyz_st(A.m + ee[q], o.m, g.wt);
      pyz_st(A.v + ee[q], o.v, g.wt);
    }
  }
}
