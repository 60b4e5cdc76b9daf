// pyz_sgld_lanes.h -- P SGLD chains that differ by their hyper-parameters ("lanes": pyz_sgld_lanes_step / _run), and the
// score of every lane on a data split (pyz_lane_scores).
//
// k_sgld_update_lanes is k_sgld_update_chains (pyz_sgld_chains.h) with two things per lane instead of per launch:
//   lr   = lr[c]                     (the chains kernel: ctl->lr for every chain)
//   seed = seed + c * seed_stride    (the chains kernel: seed + c), seed_stride in {0, 1}
// and the same float32 expressions in the same order behind them:
//   noise = lr * z;  theta[c][e] += -lr * (grad[c][e] + noise)
//   mean[c][e] <- (mean[c][e] * n + theta) / (n + 1);  sq_mean[c][e] <- (sq_mean[c][e] * n + theta^2) / (n + 1)
// With every lr[c] equal to ctl->lr and seed_stride = 1 a lanes step is a chains step bit for bit.  seed_stride = 0 gives
// every lane ONE noise stream (common random numbers): two lanes with equal starts and equal rates stay equal, and lanes
// that differ by their rates alone are compared on the same draws.
//
// The rates of a step ride in the launch's kernel arguments (a run enqueues every step as a launch of its own, so step
// s's launch carries row s of the host's (n_steps, P) table): a fixed array of PYZ_MAX_LANES floats indexed by blockIdx.y,
// no second device table and nothing to stage.  n, the batch and the loss slot still come from the StepCtl, which lane 0
// advances for the next step as chain 0 does.
//
// Layout, alignment rule (per buffer and per row, the last partial group element by element), grid and duties are those
// of the chains kernel; pyz_ld4 / pyz_st4 / pyz_row_aligned16 are its helpers.
//
// k_lane_scores: thread = row of the split, grid (ceil(n / 256), lanes).  The per-row loss is the plan's loss head's, in
// its float32 expressions, from the last layer's logits (softmax, one sigmoid unit) or outputs (MSE); a workgroup adds
// its rows in float64 (pyz_block_sum: fixed order) into ONE partial, and the workgroup of a lane that finishes last adds
// the lane's partials in workgroup order -- whichever workgroup that is, the sum is the same bits.  The hand-over is an
// integer ticket per lane (agent-scope acquire / release); no floating-point atomics anywhere.
#pragma once

#include "pyz_common.h"
#include "pyz_gemm.h"
#include "pyz_kernels.h"
#include "pyz_rng.h"
#include "pyz_sgld_chains.h"

struct LaneRates {                 // (PYZ_MAX_LANES: include/pyz.h)
  float lr[PYZ_MAX_LANES];
};

struct SgldLanesArgs {
  SgldChainsArgs c;                // seed: the base; lane c draws seed + c * seed_stride
  unsigned seed_stride;            // 0 or 1
  LaneRates rates;                 // lane c steps with rates.lr[c]
};

__global__ void __launch_bounds__(256) k_sgld_update_lanes(SgldLanesArgs a) {
  const SgldChainsArgs &g = a.c;
  const long long c = blockIdx.y;
  const float lr = a.rates.lr[c];
  const long long n = g.ctl->n;
  const float fn = (float)n, fn1 = fn + 1.0f;
  float *th_row = g.theta + c * g.D, *mu_row = g.mean + c * g.D, *sq_row = g.sq_mean + c * g.D;
  const float *gr_row = g.grad + c * g.grad_pstride;
  const float *nz_row = g.unit_noise ? g.unit_noise + c * g.D : nullptr;
  const bool a_th = pyz_row_aligned16(th_row), a_mu = pyz_row_aligned16(mu_row), a_sq = pyz_row_aligned16(sq_row);
  const bool a_gr = pyz_row_aligned16(gr_row), a_nz = nz_row && pyz_row_aligned16(nz_row);
  const uint64_t seed = g.seed + (uint64_t)c * (uint64_t)a.seed_stride;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < g.groups; t += stride) {
    const long long e0 = 4 * t;
    const long long left = g.D - e0;
    const int nv = left >= 4 ? 4 : (int)left;
    const bool full = nv == 4;
    float z[4], th[4], mu[4], sq[4], gv[4];
    if (nz_row) {
      pyz_ld4(nz_row + e0, a_nz && full, nv, z);
    } else {
      const float4 q = pyz_normal4(seed, PYZ_STREAM_SGLD, (uint32_t)n, (uint64_t)t);
      z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
    }
    pyz_ld4(th_row + e0, a_th && full, nv, th);
    pyz_ld4(gr_row + e0, a_gr && full, nv, gv);
    pyz_ld4(mu_row + e0, a_mu && full, nv, mu);
    pyz_ld4(sq_row + e0, a_sq && full, nv, sq);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float noise = lr * z[j];
      const float t1 = th[j] + (-lr) * (gv[j] + noise);
      th[j] = t1;
      mu[j] = (mu[j] * fn + t1) / fn1;
      sq[j] = (sq[j] * fn + t1 * t1) / fn1;
    }
    pyz_st4(th_row + e0, a_th && full, nv, th);
    pyz_st4(mu_row + e0, a_mu && full, nv, mu);
    pyz_st4(sq_row + e0, a_sq && full, nv, sq);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float *lo = g.loss + (g.loss_indexed ? (long long)(g.ctl->slot0 + g.ctl->i) * gridDim.y : 0);
    lo[c] = g.ploss[c];
    if (c == 0 && g.next) pyz_prepare_next(g.ctl, g.next, g.tab_bs, g.tab_lr, g.row_stride);
  }
}

// ---------------------------------------------------------------- scores
struct LaneScoreArgs {
  const float *last;               // (S, max_batch, C): the last layer's logits (SCCE, BCE) or outputs (MSE) of S lanes
  long long pstride;               // max_batch * C
  int C, loss, n;                  // rows [0, n) are scored; rows beyond are never read
  const void *y;                   // int32 labels (SCCE) / float targets (MSE: (n, C); BCE: (n, 1))
  unsigned long long *part;        // (S, nblk) float64 bits: the workgroups' loss sums
  unsigned long long *epart;       // (S, nblk) the workgroups' wrong rows
  unsigned *ticket;                // [S], zero at launch
  double *loss_sum;                // [S] out
  long long *errors;               // [S] out, may be nullptr
};

typedef __attribute__((address_space(1))) unsigned long long pyz_ls_gu64;

__global__ void __launch_bounds__(256) k_lane_scores(LaneScoreArgs g) {
  __shared__ double sm[16];
  __shared__ unsigned long long wrong[4];
  __shared__ int is_last;
  const int C = g.C, s = blockIdx.y, tid = threadIdx.x, nblk = gridDim.x;
  const int m = blockIdx.x * 256 + tid;
  double lm = 0.0;
  bool bad = false;
  if (m < g.n) {
    const float *z = g.last + s * g.pstride + (long long)m * C;
    if (g.loss == PYZ_LOSS_SCCE) {   // k_loss_scce's row: logsumexp(z) - z[y]
      const int y = reinterpret_cast<const int32_t *>(g.y)[m];
      float mx = z[0];
      int best = 0;
      for (int c = 1; c < C; ++c) {
        const float v = z[c];
        if (v > mx) best = c;        // the FIRST maximum (np.argmax)
        mx = fmaxf(mx, v);
      }
      float se = 0.0f;
      for (int c = 0; c < C; ++c) se += expf(z[c] - mx);
      const float lse = mx + logf(se);
      const float zy = (y >= 0 && y < C) ? z[y] : __builtin_nanf("");
      lm = (double)(lse - zy);
      bad = best != y;
    } else if (g.loss == PYZ_LOSS_BCE) {   // the head's row from the logit of the one unit
      const float yv = reinterpret_cast<const float *>(g.y)[m];
      float p;
      lm = (double)pyz_bce_row(z[0], yv, p);
      bad = (p > 0.5f) != (yv > 0.5f);
    } else {                         // k_loss_mse's row: mean over the outputs of (o - y)^2
      const float *y = reinterpret_cast<const float *>(g.y) + (long long)m * C;
      float acc = 0.0f;
      for (int c = 0; c < C; ++c) {
        const float e = z[c] - y[c];
        acc += e * e;
      }
      lm = (double)(acc / (float)C);
    }
  }
  const unsigned long long votes = __ballot(bad);
  if ((tid & 63) == 0) wrong[tid >> 6] = (unsigned long long)__popcll(votes);
  const double sum = pyz_block_sum(lm, sm);   // (its barriers order `wrong` as well)
  if (tid == 0) {
    const long long slot = (long long)s * nblk + blockIdx.x;
    __hip_atomic_store((pyz_ls_gu64 *)(g.part + slot), __builtin_bit_cast(unsigned long long, sum), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((pyz_ls_gu64 *)(g.epart + slot), (wrong[0] + wrong[1]) + (wrong[2] + wrong[3]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    // release my partials, acquire everybody's who came before
    const unsigned t = __hip_atomic_fetch_add(g.ticket + s, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    is_last = t == (unsigned)nblk - 1u;
  }
  __syncthreads();
  if (!is_last || tid != 0) return;
  double tot = 0.0;
  unsigned long long err = 0;
  for (int b = 0; b < nblk; ++b) {   // workgroup order, whoever adds
    const long long slot = (long long)s * nblk + b;
    tot += __builtin_bit_cast(double, __hip_atomic_load((pyz_ls_gu64 *)(g.part + slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    err += __hip_atomic_load((pyz_ls_gu64 *)(g.epart + slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  g.loss_sum[s] = tot;
  if (g.errors) g.errors[s] = g.loss == PYZ_LOSS_MSE ? 0 : (long long)err;
}
