// pyz_sgld_chains.h -- the SGLD update of P independent chains in one launch (pyz_sgld_chains_step / _run).
//
// k_sgld_update (pyz_kernels.h) over a (P, D) state.  For chain c and element e of it, with lr, n and batch read from the
// StepCtl as there:
//   noise = lr * z;  theta[c][e] += -lr * (grad[c][e] + noise)
//   mean[c][e] <- (mean[c][e] * n + theta) / (n + 1);  sq_mean[c][e] <- (sq_mean[c][e] * n + theta^2) / (n + 1)
// in the same float32 expressions, in the same order.  z = pyz_normal4(seed + c, PYZ_STREAM_SGLD, n, t) for the four-element
// group t of the CHAIN (not of the matrix), or unit_noise[c][e] when a (P, D) matrix is injected: chain c draws what a
// single-chain pyz_sgld_step with seed + c draws.
//
// Layout: theta, mean, sq_mean and unit_noise are (P, D) row-major with row stride D, grad is the plan's gradient buffer
// (row stride grad_pstride).  A thread owns one group (one Philox call), so a group's address is 16-byte aligned only when
// its row starts on a 16-byte boundary: with D % 4 != 0 that holds for every fourth row at most, and a caller's buffer may
// itself start 4 bytes off.  Whether a row of a buffer takes 16-byte accesses is decided per buffer and per chain from the
// row's address (uniform over the workgroup: blockIdx.y is the chain); the last, partial group of a row and every group
// of an unaligned row go element by element.
//
// Grid: (gx, P) workgroups of 256 threads, each striding over its chain's groups.  gx = min(ceil(groups / 256),
// max(1, 8 * CUs / P)): a launch fills the chip about once -- 8 workgroups of 4 waves per CU, i.e. 8 waves per SIMD asked
// for, of which the kernel's 51 VGPRs (103 SGPRs, no scratch, no LDS: tools/kernel_resources.py) keep 7 resident --
// instead of one workgroup per 1024 elements of every chain (P = 32 at C2 would be 5000 workgroups of one group per
// thread, each paying its own ramp) or of one chain only (155 workgroups at C2: 60 % of the CUs).  The kernel streams 7
// floats per element (theta, mean, sq_mean read and written, grad read; 8 with injected noise) and keeps nothing: no LDS,
// no reuse, so the only lever is having enough bytes in flight per CU.
//
// Duties: thread 0 of each chain's first workgroup hands the chain's loss on -- particle c's loss / batch as the gradient
// pass left it in the plan's per-particle scalars (k_wgrad_all's spare workgroup, or k_loss_finalize; both have already
// counted it for pyz_check_finite through pyz_note_loss, so it is not counted again here) -- and thread 0 of chain 0's
// prepares the next step's StepCtl when a run gives one.
#pragma once

#include "pyz_common.h"
#include "pyz_kernels.h"
#include "pyz_rng.h"

struct SgldChainsArgs {
  float *theta, *mean, *sq_mean;   // (P, D)
  const float *grad;               // (P, grad_pstride)
  long long D, grad_pstride;
  long long groups;                // ceil(D / 4)
  const StepCtl *ctl;
  StepCtl *next;                   // may be nullptr (eager step)
  const int32_t *tab_bs;
  const float *tab_lr;
  long long row_stride;
  uint64_t seed;                   // chain c: seed + c
  const float *unit_noise;         // optional injected N(0,1), (P, D)
  const float *ploss;              // [P] the gradient pass's per-particle losses (already / batch)
  float *loss;                     // eager: [P]; run: (slots, P), row ctl->slot0 + ctl->i
  int loss_indexed;
};

__device__ __forceinline__ bool pyz_row_aligned16(const float *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// four consecutive floats of a row from p; `wide`: p is 16-byte aligned and all four exist; else the first `nv`, zeros behind
__device__ __forceinline__ void pyz_ld4(const float *p, const bool wide, const int nv, float v[4]) {
  if (wide) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.0f;
  }
}

__device__ __forceinline__ void pyz_st4(float *p, const bool wide, const int nv, const float v[4]) {
  if (wide) {
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nv) p[j] = v[j];
  }
}

// Row c of the (P, D) state with the rate and the noise seed its kernel gives it, and the row's duties: everything
// k_sgld_update_chains and k_sgld_update_lanes (pyz_sgld_lanes.h) do behind those two values.  `block` is the kernel's
// blockDim.x: only a __global__ function's own read of it compiles to the plain load of the workgroup size (a device
// function's also selects the remainder size of a ragged grid, one more load ahead of the loop).
__device__ __forceinline__ void pyz_sgld_update_row(const SgldChainsArgs &g, const long long c, const float lr,
                                                    const uint64_t seed, const unsigned block) {
  const long long n = g.ctl->n;
  const float fn = (float)n, fn1 = fn + 1.0f;
  float *th_row = g.theta + c * g.D, *mu_row = g.mean + c * g.D, *sq_row = g.sq_mean + c * g.D;
  const float *gr_row = g.grad + c * g.grad_pstride;
  const float *nz_row = g.unit_noise ? g.unit_noise + c * g.D : nullptr;
  // a group starts 16 bytes x t behind its row: the row's alignment is the group's
  const bool a_th = pyz_row_aligned16(th_row), a_mu = pyz_row_aligned16(mu_row), a_sq = pyz_row_aligned16(sq_row);
  const bool a_gr = pyz_row_aligned16(gr_row), a_nz = nz_row && pyz_row_aligned16(nz_row);
  const long long stride = (long long)gridDim.x * block;
  for (long long t = (long long)blockIdx.x * block + threadIdx.x; t < g.groups; t += stride) {
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

__global__ void __launch_bounds__(256) k_sgld_update_chains(SgldChainsArgs g) {
  const long long c = blockIdx.y;
  pyz_sgld_update_row(g, c, g.ctl->lr, g.seed + (uint64_t)c, blockDim.x);
}
