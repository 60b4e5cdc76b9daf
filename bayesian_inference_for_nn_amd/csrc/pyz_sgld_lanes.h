// pyz_sgld_lanes.h -- P SGLD chains that differ by their hyper-parameters ("lanes": pyz_sgld_lanes_step / _run), and the
// score of every lane on a data split (pyz_lane_scores).
//
// k_sgld_update_lanes runs the chains kernel's body, pyz_sgld_update_row (pyz_sgld_chains.h: expressions, layout,
// alignment rule, grid and duties are described there), with two things per lane instead of per launch:
//   lr   = lr[c]                     (the chains kernel: ctl->lr for every chain)
//   seed = seed + c * seed_stride    (the chains kernel: seed + c), seed_stride in {0, 1}
// With every lr[c] equal to ctl->lr and seed_stride = 1 a lanes step is a chains step bit for bit.  seed_stride = 0 gives
// every lane ONE noise stream (common random numbers): two lanes with equal starts and equal rates stay equal, and lanes
// that differ by their rates alone are compared on the same draws.
//
// The rates of a step ride in the launch's kernel arguments (a run enqueues every step as a launch of its own, so step
// s's launch carries row s of the host's (n_steps, P) table): a fixed array of PYZ_MAX_LANES floats indexed by blockIdx.y,
// no second device table and nothing to stage.  n, the batch and the loss slot still come from the StepCtl, which lane 0
// advances for the next step as chain 0 does.
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
  const long long c = blockIdx.y;
  pyz_sgld_update_row(a.c, c, a.rates.lr[c], a.c.seed + (uint64_t)c * (uint64_t)a.seed_stride, blockDim.x);
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
