// pyz_members.h -- the SGD / SWAG update of P ensemble members in one launch (pyz_sgd_members_step / _run,
// pyz_swag_members_step / _run): deep ensembles and MultiSWAG train their P networks in one particle-batched step.
//
// k_members_update stands behind the particle-batched gradient pass where k_sgld_update_chains (pyz_sgld_chains.h) stands
// for SGLD chains, and is that kernel without the noise and with the gated bookkeeping of SGD.py / SWAG.py.  For member c
// and element e of it, with lr and n read from the StepCtl, in one of two modes that is the same for the whole launch:
//
//   SGD rows   th = fmaf(-lr, g, th0)
//              hit step:  mean[c][e] = th        (SGD.py:78-84: the "mean" is the weights after the last hit step)
//   SWAG rows  th = fmaf(-lr, g, th0)
//              hit step:  mu = (mu0 * fn + th) / fn1;  sq = fmaf(th, th, sq0 * fn) / fn1;  dev = th - mu
//                         (fn = (float)n, fn1 = fn + 1) -- dev goes to one column of the member's deviation block
//
// These are the float32 expressions of pyz_update_math's PYZ_UPD_SGD and PYZ_UPD_SWAG arms (pyz_fused.h), restated here
// in that order with contraction off: fmaf is one rounding, everything else rounds per operation.  They are restated, not
// shared, because the code around those arms moves their roundings ("The serial head and tail").
//
// A hit step is one whose count is a multiple of `frequency`.  A run (freq > 0) decides it from ctl->n on the device and
// writes the deviation to column min(ceil(n / freq), k - 1): columns are appended until there are k, afterwards the LAST one
// is replaced (SWAG.py:85-89, as written).  An eager step (freq == 0) takes the caller's flag `hit` and the caller's
// column `col`; col < 0 writes no deviation (pyz_swag_step's dev_row = NULL).  On a step that is no hit the kernel neither
// reads nor writes mean, sq_mean or the deviations.
//
// Layout: theta, mean, sq_mean are (P, D) row-major with row stride D, grad is the plan's gradient buffer (row stride
// grad_pstride), the deviations are (P, k, D) row-major: member stride k * D, column stride D.  Whether a row of a buffer
// takes 16-byte accesses is decided per buffer and per member from the row's address, as in pyz_sgld_update_row -- the
// member's deviation column has an alignment of its own --; the last, partial group of a row and every group of an
// unaligned row go element by element.
//
// Grid: (gx, P) workgroups of 256 threads from sgld_rows_grid, blockIdx.y the member, a thread striding over the
// four-element groups of its member's row.  The kernel streams 3 floats per element on a step that is no hit (theta read
// and written, grad read), 4 on an SGD hit, 8 on a SWAG hit (mean and sq_mean read and written, the deviation written);
// no RNG, no LDS, nothing is reused.
//
// Duties, as pyz_sgld_update_row's: thread 0 of each member's first workgroup hands the member's loss on (ploss[c], which
// the gradient pass has already counted for pyz_check_finite), thread 0 of member 0's prepares the next step's StepCtl
// when a run gives one.
#pragma once

#include "pyz_common.h"
#include "pyz_kernels.h"
#include "pyz_sgld_chains.h"   // pyz_row_aligned16, pyz_ld4, pyz_st4

struct MembersArgs {
  float *theta, *mean;             // (P, D)
  float *sq_mean;                  // (P, D), SWAG rows only
  float *dev;                      // (P, k, D), SWAG rows only
  const float *grad;               // (P, grad_pstride)
  long long D, grad_pstride;
  long long groups;                // ceil(D / 4)
  const StepCtl *ctl;
  StepCtl *next;                   // may be nullptr (eager step)
  const int32_t *tab_bs;
  const float *tab_lr;
  long long row_stride;
  const float *ploss;              // [P] the gradient pass's per-particle losses (already / batch)
  float *loss;                     // eager: [P]; run: (slots, P), row ctl->slot0 + ctl->i
  int loss_indexed;
  int swag;                        // 0: SGD rows, 1: SWAG rows
  int k;                           // deviation columns of a member
  int freq;                        // run: > 0, hit and column follow from ctl->n; eager step: 0, `hit` and `col` hold
  int hit, col;                    // eager step: the caller's flag and column (col < 0: no deviation is written)
};

template <bool SWAG>
__device__ __forceinline__ void pyz_members_update_row(const MembersArgs &g, const long long c, const unsigned block) {
#pragma clang fp contract(off)
  const long long n = g.ctl->n;
  const float lr = g.ctl->lr;
  const bool hit = g.freq > 0 ? (n % g.freq == 0) : (g.hit != 0);
  const long long col = g.freq > 0 ? min((n + g.freq - 1) / g.freq, (long long)g.k - 1) : (long long)g.col;
  const float fn = (float)n, fn1 = fn + 1.0f;
  float *th_row = g.theta + c * g.D, *mu_row = g.mean + c * g.D;
  float *sq_row = SWAG ? g.sq_mean + c * g.D : nullptr;
  float *dv_row = SWAG && hit && col >= 0 ? g.dev + (c * g.k + col) * g.D : nullptr;
  const float *gr_row = g.grad + c * g.grad_pstride;
  // a group starts 16 bytes x t behind its row: the row's alignment is the group's
  const bool a_th = pyz_row_aligned16(th_row), a_mu = pyz_row_aligned16(mu_row), a_gr = pyz_row_aligned16(gr_row);
  const bool a_sq = SWAG && pyz_row_aligned16(sq_row), a_dv = dv_row && pyz_row_aligned16(dv_row);
  const long long stride = (long long)gridDim.x * block;
  for (long long t = (long long)blockIdx.x * block + threadIdx.x; t < g.groups; t += stride) {
    const long long e0 = 4 * t;
    const long long left = g.D - e0;
    const int nv = left >= 4 ? 4 : (int)left;
    const bool full = nv == 4;
    float th[4], gv[4];
    pyz_ld4(th_row + e0, a_th && full, nv, th);
    pyz_ld4(gr_row + e0, a_gr && full, nv, gv);
#pragma unroll
    for (int j = 0; j < 4; ++j) th[j] = __builtin_fmaf(-lr, gv[j], th[j]);
    pyz_st4(th_row + e0, a_th && full, nv, th);
    if (!hit) continue;
    if (!SWAG) {
      pyz_st4(mu_row + e0, a_mu && full, nv, th);
      continue;
    }
    float mu[4], sq[4], dv[4];
    pyz_ld4(mu_row + e0, a_mu && full, nv, mu);
    pyz_ld4(sq_row + e0, a_sq && full, nv, sq);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mu[j] = (mu[j] * fn + th[j]) / fn1;
      sq[j] = __builtin_fmaf(th[j], th[j], sq[j] * fn) / fn1;
      dv[j] = th[j] - mu[j];
    }
    pyz_st4(mu_row + e0, a_mu && full, nv, mu);
    pyz_st4(sq_row + e0, a_sq && full, nv, sq);
    if (dv_row) pyz_st4(dv_row + e0, a_dv && full, nv, dv);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float *lo = g.loss + (g.loss_indexed ? (long long)(g.ctl->slot0 + g.ctl->i) * gridDim.y : 0);
    lo[c] = g.ploss[c];
    if (c == 0 && g.next) pyz_prepare_next(g.ctl, g.next, g.tab_bs, g.tab_lr, g.row_stride);
  }
}

__global__ void __launch_bounds__(256) k_members_update(MembersArgs g) {
  const long long c = blockIdx.y;
  if (g.swag)
    pyz_members_update_row<true>(g, c, blockDim.x);
  else
    pyz_members_update_row<false>(g, c, blockDim.x);
}
