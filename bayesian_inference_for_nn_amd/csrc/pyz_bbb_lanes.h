// pyz_bbb_lanes.h -- P Bayes-by-Backprop posteriors that differ by their hyper-parameters ("lanes": pyz_bbb_lanes_step /
// _run): the two ends of pyz_bbb_step for a (P, D) state, around the particle-batched gradient pass.
//
// k_bbb_sample_lanes is k_bbb_sample and k_bbb_update_lanes is k_bbb_update (pyz_kernels.h: expressions and their
// reference lines are there), in the same float32 expressions and the same order, for row c of the state with
//   lr = lr[c], alpha = alpha[c], prior = (prior_mean[c], softplus(prior_rho[c]))   (or the shared per-element vectors)
//   eps = pyz_normal4(seed + c * seed_stride, PYZ_STREAM_BBB, step, t), t the four-element group of the ROW, or row c of
//         the injected (P, D) matrix; the update kernel recomputes what the sample kernel drew.
// seed_stride = 0 gives every lane ONE noise stream (lanes differ by their hyper-parameters alone), 1 gives lane c the
// stream of a single pyz_bbb_step with seed + c (repeats of one point as lanes).
//
// Layout (pyz_sgld_chains.h): mu, rho, w and eps are (P, D) row-major with row stride D, the gradient is the plan's buffer
// with its own row stride.  Lane = blockIdx.y.  A thread owns one group (one Philox call); whether a row of a buffer
// takes 16-byte accesses is decided per buffer and per lane from the row's address (pyz_ld4 / pyz_st4).
//
// The hyper-parameters ride in the launch's kernel arguments, as LaneRates does for SGLD (pyz_sgld_lanes.h): four fixed
// arrays of PYZ_MAX_LANES floats indexed by blockIdx.y, no second device table.  The step number is the launch's
// argument (eager) or ctl->n (run), as BbbArgs.chained has it.
//
// log q - log p: summed in float64, ONE partial per fixed block of 1024 consecutive elements of the row (256 groups,
// pyz_block_sum), stored at (c, b), b < ceil(groups / 256) -- whichever workgroup walks block b.  The grid
// (sgld_rows_grid: the chip filled about once over all P rows) therefore does not show in the sum: a lane's w and its
// log q - log p are the bits pyz_bbb_step gives from the same (mu, rho, eps, prior).  A workgroup's loop runs over
// blocks, uniformly for all of its threads (pyz_block_sum has barriers); a thread past the row's last group adds zero.
//
// Duties of the update kernel: wave 0 of each lane's first workgroup adds the lane's partials in the fixed order of
// pyz_sum_partials and its first thread writes {loss + alpha_c kl, loss, kl, 0} with loss = particle c's loss / batch as
// the gradient pass left it in the plan's per-particle scalars -- to cost[4 c ..] (eager) or to row ctl->slot0 + ctl->i
// of (slots, P, 4) (run) -- and counts a non-finite cost (pyz_note_loss); lane 0's prepares the next StepCtl in a run.
// No atomics on floating-point values: the same call gives the same bits.
//
// Both kernels stream (sample: 2 floats read, 1 written per element; update: 4 read, 2 written, plus injected eps) and
// carry several transcendentals per element; the lane's softplus(prior_rho), its logarithm and its inverse square are
// taken once per thread.
#pragma once

#include "pyz_common.h"
#include "pyz_kernels.h"
#include "pyz_rng.h"
#include "pyz_sgld_chains.h"

struct BbbLaneTable {              // (PYZ_MAX_LANES: include/pyz.h)
  float lr[PYZ_MAX_LANES], alpha[PYZ_MAX_LANES], prior_mean[PYZ_MAX_LANES], prior_rho[PYZ_MAX_LANES];
};

struct BbbLanesArgs {
  float *mu, *rho, *w;             // (P, D)
  const float *grad;               // (P, grad_pstride)
  long long D, grad_pstride;
  long long groups;                // ceil(D / 4)
  int nblk;                        // ceil(groups / 256): the log q - log p partials of a lane
  const float *pm_vec, *pr_vec;    // optional per-element prior mean / rho (D), shared by the lanes; else the lane's scalars
  uint64_t seed;                   // the base; lane c draws seed + c * seed_stride
  unsigned seed_stride;            // 0 or 1
  uint32_t step;                   // eager: the Philox step
  int chained;                     // run: the Philox step is ctl->n, the cost goes to row ctl->slot0 + ctl->i
  const float *eps;                // optional injected N(0,1), (P, D)
  double *part_kl;                 // (P, nblk)
  const float *ploss;              // [P] the gradient pass's per-particle losses (already / batch)
  const StepCtl *ctl;
  StepCtl *next;                   // may be nullptr (eager step)
  const int32_t *tab_bs;
  const float *tab_lr;
  long long row_stride;
  float *cost;                     // eager: (P, 4); run: (slots, P, 4)
  int *nonfinite;
  BbbLaneTable tab;
};

// the four eps of group t of lane c's row
__device__ __forceinline__ void pyz_bbb_lane_eps(const float *ez_row, const bool a_ez, const uint64_t seed,
                                                 const uint32_t step, const long long t, const int nv, float z[4]) {
  if (ez_row) {
    pyz_ld4(ez_row + 4 * t, a_ez && nv == 4, nv, z);
  } else {
    const float4 q = pyz_normal4(seed, PYZ_STREAM_BBB, step, (uint64_t)t);
    z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
  }
}

__global__ void __launch_bounds__(256) k_bbb_sample_lanes(BbbLanesArgs g) {
  __shared__ double sm[16];
  const long long c = blockIdx.y;
  const float *mu_row = g.mu + c * g.D, *rho_row = g.rho + c * g.D;
  float *w_row = g.w + c * g.D;
  const float *ez_row = g.eps ? g.eps + c * g.D : nullptr;
  const bool a_mu = pyz_row_aligned16(mu_row), a_rho = pyz_row_aligned16(rho_row), a_w = pyz_row_aligned16(w_row);
  const bool a_ez = ez_row && pyz_row_aligned16(ez_row);
  const uint64_t seed = g.seed + (uint64_t)c * (uint64_t)g.seed_stride;
  const uint32_t step = g.chained ? (uint32_t)g.ctl->n : g.step;
  const float pmean_s = g.tab.prior_mean[c];
  const float sp_s = pyz_softplus(g.tab.prior_rho[c]), lsp_s = logf(sp_s);
  for (int b = blockIdx.x; b < g.nblk; b += gridDim.x) {   // (uniform: every thread of the workgroup walks the same blocks)
    const long long t = (long long)b * 256 + threadIdx.x;
    double kl = 0.0;
    if (t < g.groups) {
      const long long e0 = 4 * t;
      const long long left = g.D - e0;
      const int nv = left >= 4 ? 4 : (int)left;
      const bool full = nv == 4;
      float z[4], mv[4], rv[4], wv[4];
      pyz_bbb_lane_eps(ez_row, a_ez, seed, step, t, nv, z);
      pyz_ld4(mu_row + e0, a_mu && full, nv, mv);
      pyz_ld4(rho_row + e0, a_rho && full, nv, rv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wv[j] = 0.0f;
        if (j < nv) {
          const long long e = e0 + j;
          const float pmean = g.pm_vec ? g.pm_vec[e] : pmean_s;
          float sp = sp_s, lsp = lsp_s;
          if (g.pr_vec) {   // uniform
            sp = pyz_softplus(g.pr_vec[e]);
            lsp = logf(sp);
          }
          const float mu = mv[j], sg = pyz_softplus(rv[j]);
          const float w = z[j] * sg + mu;
          wv[j] = w;
          const float a = (w - mu) / sg, b2 = (w - pmean) / sp;
          const float lq = -0.5f * a * a - logf(sg) - PYZ_LOG_SQRT_2PI;
          const float lp = -0.5f * b2 * b2 - lsp - PYZ_LOG_SQRT_2PI;
          kl += (double)lq - (double)lp;
        }
      }
      pyz_st4(w_row + e0, a_w && full, nv, wv);
    }
    const double s = pyz_block_sum(kl, sm);
    if (threadIdx.x == 0) g.part_kl[c * g.nblk + b] = s;
  }
}

__global__ void __launch_bounds__(256) k_bbb_update_lanes(BbbLanesArgs g) {
  const long long c = blockIdx.y;
  float *mu_row = g.mu + c * g.D, *rho_row = g.rho + c * g.D;
  const float *w_row = g.w + c * g.D, *gr_row = g.grad + c * g.grad_pstride;
  const float *ez_row = g.eps ? g.eps + c * g.D : nullptr;
  const bool a_mu = pyz_row_aligned16(mu_row), a_rho = pyz_row_aligned16(rho_row), a_w = pyz_row_aligned16(w_row);
  const bool a_gr = pyz_row_aligned16(gr_row), a_ez = ez_row && pyz_row_aligned16(ez_row);
  const uint64_t seed = g.seed + (uint64_t)c * (uint64_t)g.seed_stride;
  const uint32_t step = g.chained ? (uint32_t)g.ctl->n : g.step;
  const float lr = g.tab.lr[c], alpha = g.tab.alpha[c], pmean_s = g.tab.prior_mean[c];
  const float sp_s = pyz_softplus(g.tab.prior_rho[c]), isp2_s = 1.0f / (sp_s * sp_s);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < g.groups; t += stride) {
    const long long e0 = 4 * t;
    const long long left = g.D - e0;
    const int nv = left >= 4 ? 4 : (int)left;
    const bool full = nv == 4;
    float z[4], mv[4], rv[4], wv[4], gv[4];
    pyz_bbb_lane_eps(ez_row, a_ez, seed, step, t, nv, z);
    pyz_ld4(mu_row + e0, a_mu && full, nv, mv);
    pyz_ld4(rho_row + e0, a_rho && full, nv, rv);
    pyz_ld4(w_row + e0, a_w && full, nv, wv);
    pyz_ld4(gr_row + e0, a_gr && full, nv, gv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nv) {
        const long long e = e0 + j;
        const float pmean = g.pm_vec ? g.pm_vec[e] : pmean_s;
        float isp2 = isp2_s;
        if (g.pr_vec) {   // uniform
          const float sp = pyz_softplus(g.pr_vec[e]);
          isp2 = 1.0f / (sp * sp);
        }
        const float mu = mv[j], rho = rv[j], w = wv[j];
        const float sg = pyz_softplus(rho), sig = pyz_sigmoid(rho);
        const float d = w - mu, is2 = 1.0f / (sg * sg);
        const float g_mu = alpha * d * is2;
        const float g_rho = alpha * (-1.0f / sg + d * d * is2 / sg) * sig;
        const float g_w = gv[j] + alpha * (-d * is2 + (w - pmean) * isp2);
        mv[j] = mu - lr * (g_mu + g_w);
        rv[j] = rho - lr * (z[j] * sig * g_w + g_rho);
      }
    }
    pyz_st4(mu_row + e0, a_mu && full, nv, mv);
    pyz_st4(rho_row + e0, a_rho && full, nv, rv);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const double sk = pyz_sum_partials(g.part_kl + c * g.nblk, g.nblk);
    if (threadIdx.x == 0) {
      const float loss = g.ploss[c], kl = (float)sk;
      float *co = g.cost + (g.chained ? (long long)(g.ctl->slot0 + g.ctl->i) * gridDim.y * 4 : 0) + 4 * c;
      co[0] = loss + alpha * kl;
      pyz_note_loss(g.nonfinite, co[0]);
      co[1] = loss;
      co[2] = kl;
      co[3] = 0.0f;
      if (c == 0 && g.next) pyz_prepare_next(g.ctl, g.next, g.tab_bs, g.tab_lr, g.row_stride);
    }
  }
}
