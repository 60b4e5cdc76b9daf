// pyz_fsvi.h -- function-space variational inference (Pyesian/optimizers/FSVI.py:60-147, DESIGN assumption A8) and the
// batched float64 symmetric positive-definite solve both of its terms need.
//
// One step (pyz_fsvi_step, k particles, b batch rows, B measurement rows, n = b + B, F inputs, D weights):
//   k_fsvi_inputs        Xp (k, n, F): batch rows + z_i, measurement rows + (z_0 + ... + z_i)        FSVI.py:86-89,106,197-212
//   forward              f_i = model(W_i; Xp_i), the particle-batched Dense kernels (per-particle input)  FSVI.py:91,108
//   k_fsvi_gram          K_i = exp(-|x_r - x_s|^2 / 2) + 1e-6 I in float64, rhs = f_i                 FSVI.py:149-157
//   k_fsvi_stein_system  K_w + 1e-3 I and rhs over the D weights of W_i as scalar points, float64      FSVI.py:177-195
//   k_spd_solve_f64      alpha_i = K_i^-1 f_i and (K_w + 1e-3 I)^-1 rhs, one workgroup per system      FSVI.py:160-163,195
//   k_fsvi_delta         the merged output delta, the loss partial, and the last layer's backward pass FSVI.py:95-98,111
//   backward             k_dense_bwd_data / k_dense_bwd_weight for the layers below                      FSVI.py:96,111
//   k_fsvi_update        g, Keras legacy Adam on mu, the redraw W_i = mu + eps_i, the returned loss     FSVI.py:115-138,228-231
// Every sum runs in one fixed order: the bits of a step do not change from call to call.
#pragma once

#include "pyz_common.h"
#include "pyz_gemm.h"
#include "pyz_kernels.h"
#include "pyz_rng.h"

#define PYZ_FSVI_MAX_N 1024  // batch + measurement rows of one step
#define PYZ_FSVI_MAX_D 2048  // weights: the Stein system is D x D float64 per particle
#define PYZ_SPD_MAX_N 2048   // pyz_spd_solve_f64
#define PYZ_SPD_LDS_N 128    // systems up to this size are factorised inside LDS
#define PYZ_SPD_THREADS 1024

// the uniform of ONE element e of a Philox stream: word e % 4 of counter e / 4 (oracle/philox.py: uniform)
__device__ __forceinline__ float pyz_uniform1(uint64_t seed, uint32_t stream, uint32_t step, uint64_t e) {
  const uint64_t idx4 = e >> 2;
  const uint4 r = philox4x32_10(make_uint4((uint32_t)idx4, (uint32_t)(idx4 >> 32), step, stream),
                                make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  const uint32_t w = (e & 2) ? ((e & 1) ? r.w : r.z) : ((e & 1) ? r.y : r.x);
  return pyz_unit(w);
}

// ---------------------------------------------------------------- inputs (FSVI.py:86-89, 106, 197-212)
struct FsviInputs {
  const float *x;           // (rows, F) training split
  const int32_t *row_idx;   // the b batch rows (NULL: rows 0 .. b - 1)
  const float *lo, *hi;     // (F) per-feature min / max of the training split
  const float *xm;          // optional (B, F) measurement set; NULL: lo + u (hi - lo), u from (seed, 9, 4t)
  const float *noise;       // optional (k, F) z_i; NULL: 0.1 N(0, 1) from (seed, 9, 4t + 1), element i F + c
  float *xp;                // (k, n, F)
  int k, b, B, F;
  uint64_t seed;
  uint32_t t4;              // 4 t
};

__device__ __forceinline__ float pyz_fsvi_z(const FsviInputs &g, const int i, const int c) {
#pragma clang fp contract(off)
  if (g.noise) return g.noise[(long long)i * g.F + c];
  return 0.1f * pyz_normal1(g.seed, PYZ_STREAM_FSVI, g.t4 + 1u, (uint64_t)i * g.F + c);
}

// one thread per element of Xp; the prefix sum c_i = z_0 + ... + z_i is a sequential float32 sum from j = 0 (the
// reference's X_M += noise accumulates over its particle loop, FSVI.py:89)
__global__ void __launch_bounds__(256) k_fsvi_inputs(FsviInputs g) {
#pragma clang fp contract(off)
  const int n = g.b + g.B;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)g.k * n * g.F) return;
  const int c = (int)(e % g.F);
  const int r = (int)((e / g.F) % n);
  const int i = (int)(e / ((long long)g.F * n));
  float v;
  if (r < g.b) {
    const long long row = g.row_idx ? g.row_idx[r] : r;
    v = g.x[row * g.F + c] + pyz_fsvi_z(g, i, c);
  } else {
    const int q = r - g.b;
    float xm;
    if (g.xm) {
      xm = g.xm[(long long)q * g.F + c];
    } else {
      const float u = pyz_uniform1(g.seed, PYZ_STREAM_FSVI, g.t4, (uint64_t)q * g.F + c);
      const float lo = g.lo[c], span = g.hi[c] - lo;
      xm = lo + u * span;
    }
    float cs = pyz_fsvi_z(g, 0, c);
    for (int j = 1; j <= i; ++j) cs = cs + pyz_fsvi_z(g, j, c);
    v = xm + cs;
  }
  g.xp[e] = v;
}

// ---------------------------------------------------------------- GP prior system (FSVI.py:149-157)
// K_i[r][s] = exp(-|x_r - x_s|^2 / 2) + 1e-6 [r = s], float64 on the float32 inputs, the squared distance summed over
// the features in ascending order; column 0's threads also copy f_i into the right-hand side.
__global__ void __launch_bounds__(256) k_fsvi_gram(const float *xp, const int n, const int F, const float *f,
                                                   const long long f_pstride, double *gram, double *rhs, float *f_out) {
  const int i = blockIdx.y;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)n * n) return;
  const int r = (int)(e / n), s = (int)(e % n);
  const float *xr = xp + ((long long)i * n + r) * F, *xs = xp + ((long long)i * n + s) * F;
  double d2 = 0.0;
  for (int c = 0; c < F; ++c) {
    const double d = (double)xr[c] - (double)xs[c];
    d2 = fma(d, d, d2);
  }
  gram[(long long)i * n * n + e] = exp(-0.5 * d2) + (r == s ? 1e-6 : 0.0);
  if (s == 0) {
    const float fr = f[i * f_pstride + r];
    rhs[(long long)i * n + r] = (double)fr;
    if (f_out) f_out[(long long)i * n + r] = fr;
  }
}

// ---------------------------------------------------------------- Stein system (FSVI.py:177-195)
// Row a of particle i: K_w[a][c] = exp(-(w_a - w_c)^2 / 2) (+ 1e-3 on the diagonal) and
// rhs_a = (1 / D) sum_c -(w_a - w_c) K_w[a][c].  One workgroup per row; thread t sums its columns t, t + 256, ... in
// ascending order, the 256 partial sums are added by a fixed tree.
__global__ void __launch_bounds__(256) k_fsvi_stein_system(const float *w, const int D, double *km, double *rhs) {
  __shared__ double red[256];
  const int a = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  const float *wi = w + (long long)i * D;
  const double wa = (double)wi[a];
  double *row = km + ((long long)i * D + a) * D;
  double s = 0.0;
  for (int c = tid; c < D; c += 256) {
    const double d = wa - (double)wi[c];
    const double kv = exp(-0.5 * d * d);
    row[c] = kv + (c == a ? 1e-3 : 0.0);
    s = fma(-d, kv, s);
  }
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) rhs[(long long)i * D + a] = red[0] / (double)D;
}

// ---------------------------------------------------------------- batched SPD solve, float64
// One workgroup per system: in-place lower Cholesky A = L L^T (right-looking), then L y = b and L^T x = y.  LDS_A: the
// matrix is copied into LDS (row stride n | 1: a column walk touches every bank) and factorised there column by column --
// n <= PYZ_SPD_LDS_N, 132 KiB; else it is factorised in panels where it lies in global memory by the same workgroup
// (pyz_spd_blocked).  a holds L afterwards only on the global path (the LDS copy is not written back: callers want the
// solution).  A pivot that is not positive (NaN included) sets fail[system] and fills the solution with NaN: every thread
// reads the same pivot behind a barrier, so the exit is uniform.  No spin waits, no traffic between workgroups.
// The global-memory path (n > PYZ_SPD_LDS_N), right-looking in panels of nb columns (32 up to n = 512, 16 up to 1024, else 4: the
// panel's rows, n x (nb + 1) doubles, must fit LDS beside the two vectors).  Per panel: its columns are read into LDS once;
// factorised there column by column behind LDS-only barriers, with the forward substitution of the same column riding along
// (y_j = b_j / L_jj, b_r -= L_rj y_j: the column is final the moment it is scaled); written back; then ONE rank-nb update of
// the trailing lower triangle in global memory (a wave per row, lanes along the columns, both factors from LDS).  The chain
// of dependent global round trips is one per panel instead of several per column.  The back substitution sweeps the rows
// of L from the last: PYZ_SPD_PF rows are requested at a time into registers, the sweep over them waits on LDS only.
#define PYZ_SPD_PF 8
__host__ __device__ static inline int pyz_spd_panel(int n) { return n <= 512 ? 32 : (n <= 1024 ? 16 : 4); }

__device__ __forceinline__ bool pyz_spd_blocked(double *ag, double *rhs, const int n, const int nb, double *lds) {
  const int tid = threadIdx.x, T = blockDim.x, wv = tid >> 6, ln = tid & 63, W = T >> 6;
  const int sh = nb == 32 ? 5 : (nb == 16 ? 4 : 2), ps = nb + 1;   // row stride nb + 1: a column walk touches every bank
  double *bb = lds, *yy = lds + n, *P = lds + 2 * n;
  for (int r = tid; r < n; r += T) bb[r] = rhs[r];
  for (int j0 = 0; j0 < n; j0 += nb) {
    const int w = min(nb, n - j0), m = n - j0;
    __syncthreads();                                  // the trailing update of the panel before is in memory; P is free
    for (int e = tid; e < m * nb; e += T) {
      const int r = e >> sh, c = e & (nb - 1);
      if (c < w) P[r * ps + c] = ag[(long long)(j0 + r) * n + j0 + c];
    }
    for (int jj = 0; jj < w; ++jj) {
      pyz_lds_barrier();                              // column jj has every update of the columns before it
      const double d = P[jj * ps + jj];
      if (!(d > 0.0)) return false;                   // the same value in every thread
      const double sd = sqrt(d);
      const double yj = bb[j0 + jj] / sd;
      for (int r = jj + 1 + tid; r < m; r += T) P[r * ps + jj] /= sd;
      pyz_lds_barrier();
      if (tid == 0) {                                 // (nobody reads the pivot or b_j again)
        P[jj * ps + jj] = sd;
        yy[j0 + jj] = yj;
      }
      for (int r = jj + 1 + tid; r < m; r += T) bb[j0 + r] = fma(-P[r * ps + jj], yj, bb[j0 + r]);
      const int c = jj + 1 + (tid & (nb - 1));        // the rest of the panel: lanes along its columns
      if (c < w) {
        const double lc = P[c * ps + jj];
        for (int r = jj + 1 + (tid >> sh); r < m; r += T >> sh)
          if (c <= r) P[r * ps + c] = fma(-P[r * ps + jj], lc, P[r * ps + c]);
      }
    }
    __syncthreads();
    for (int e = tid; e < m * nb; e += T) {           // L's columns of this panel (the back substitution reads them)
      const int r = e >> sh, c = e & (nb - 1);
      if (c < w && c <= r) ag[(long long)(j0 + r) * n + j0 + c] = P[r * ps + c];
    }
    for (int r = w + wv; r < m; r += W) {             // A[r][c] -= sum_t L[r][t] L[c][t] over the panel's columns t
      const double *pr = P + r * ps;
      double *ar = ag + (long long)(j0 + r) * n + j0;
      for (int c = w + ln; c <= r; c += 64) {
        const double *pc = P + c * ps;
        double acc = ar[c];
        for (int t = 0; t < w; ++t) acc = fma(-pr[t], pc[t], acc);
        ar[c] = acc;
      }
    }
  }
  __syncthreads();                                    // L is in memory, y in yy
  for (int jb = n - 1; jb >= 0; jb -= PYZ_SPD_PF) {    // L^T x = y: row j of L is column j of L^T
    double row[PYZ_SPD_PF][2], dg[PYZ_SPD_PF];
#pragma unroll
    for (int u = 0; u < PYZ_SPD_PF; ++u) {
      const int j = jb - u;
      dg[u] = j >= 0 ? ag[(long long)j * n + j] : 1.0;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = tid + q * T;
        row[u][q] = (j >= 0 && c < j) ? ag[(long long)j * n + c] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < PYZ_SPD_PF; ++u) {
      const int j = jb - u;
      if (j >= 0) {                                   // (uniform)
        pyz_lds_barrier();
        const double xj = yy[j] / dg[u];
        if (tid == 0) rhs[j] = xj;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int c = tid + q * T;
          if (c < j) yy[c] = fma(-row[u][q], xj, yy[c]);
        }
      }
    }
  }
  return true;
}

template <bool LDS_A>
__global__ void __launch_bounds__(PYZ_SPD_THREADS) k_spd_solve_f64(double *a_all, double *rhs_all, const int n, int *fail) {
  extern __shared__ double spd_lds[];
  const int tid = threadIdx.x, T = blockDim.x, sys = blockIdx.x;
  double *col = spd_lds, *bb = spd_lds + n, *yy = spd_lds + 2 * n;
  double *ag = a_all + (long long)sys * n * n, *rhs = rhs_all + (long long)sys * n;
  if constexpr (!LDS_A) {
    const bool ok = pyz_spd_blocked(ag, rhs, n, pyz_spd_panel(n), spd_lds);   // (T = PYZ_SPD_THREADS >= n / 2)
    if (!ok) {
      __syncthreads();
      for (int r = tid; r < n; r += T) rhs[r] = __builtin_nan("");
    }
    if (tid == 0 && fail) fail[sys] = ok ? 0 : 1;
    return;
  }
  const int ld = n | 1;
  double *A = spd_lds + 3 * n;
  for (int e = tid; e < n * n; e += T) A[(e / n) * ld + (e % n)] = ag[e];
  for (int r = tid; r < n; r += T) bb[r] = rhs[r];
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    __syncthreads();                               // column j has every update of the columns before it
    const double d = A[(long long)j * ld + j];
    if (!(d > 0.0)) {                              // the same value in every thread
      bad = true;
      break;
    }
    const double sd = sqrt(d);
    for (int r = j + tid; r < n; r += T) col[r] = r == j ? sd : A[(long long)r * ld + j] / sd;
    __syncthreads();
    for (int r = j + tid; r < n; r += T) A[(long long)r * ld + j] = col[r];
    // trailing update of the lower triangle: A[r][c] -= L[r][j] L[c][j], j < c <= r; a wave takes a row, its lanes the columns
    const int wv = tid >> 6, ln = tid & 63, W = T >> 6;
    for (int r = j + 1 + wv; r < n; r += W) {
      const double lr = col[r];
      double *ar = A + (long long)r * ld;
      for (int c = j + 1 + ln; c <= r; c += 64) ar[c] = fma(-lr, col[c], ar[c]);
    }
  }
  if (bad) {
    for (int r = tid; r < n; r += T) rhs[r] = __builtin_nan("");
    if (tid == 0 && fail) fail[sys] = 1;
    return;
  }
  // L y = b: column sweep; bb[j] is final when column j is reached (only rows below j are written in sweep j)
  for (int j = 0; j < n; ++j) {
    __syncthreads();
    const double yj = bb[j] / A[(long long)j * ld + j];
    if (tid == 0) yy[j] = yj;
    for (int r = j + 1 + tid; r < n; r += T) bb[r] = fma(-A[(long long)r * ld + j], yj, bb[r]);
  }
  // L^T x = y: row j of L is column j of L^T
  for (int j = n - 1; j >= 0; --j) {
    __syncthreads();
    const double xj = yy[j] / A[(long long)j * ld + j];
    if (tid == 0) rhs[j] = xj;
    const double *aj = A + (long long)j * ld;
    for (int c = tid; c < j; c += T) yy[c] = fma(-aj[c], xj, yy[c]);
  }
  if (tid == 0 && fail) fail[sys] = 0;
}

static inline size_t pyz_spd_lds_bytes(int n) {
  if (n <= PYZ_SPD_LDS_N) return sizeof(double) * ((size_t)3 * n + (size_t)(n | 1) * n);
  return sizeof(double) * ((size_t)2 * n + (size_t)n * (pyz_spd_panel(n) + 1));   // at most 152 KiB (n = 1024)
}

// the allowance for more than 64 KiB of dynamic LDS is a per-device attribute of the function
static inline int pyz_spd_prepare() {
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_spd_solve_f64<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)pyz_spd_lds_bytes(PYZ_SPD_LDS_N)) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void *>(k_spd_solve_f64<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)pyz_spd_lds_bytes(1024)) != hipSuccess)
    return pyz_fail(PYZ_E_HIP, "hipFuncSetAttribute(k_spd_solve_f64) failed");
  return PYZ_OK;
}

static inline void pyz_launch_spd(double *a, double *rhs, int n, int n_systems, int *fail, hipStream_t st) {
  const size_t lds = pyz_spd_lds_bytes(n);
  // small systems: a column has fewer rows than a large workgroup has waves
  const int threads = n <= 32 ? 256 : PYZ_SPD_THREADS;
  if (n <= PYZ_SPD_LDS_N) PYZ_LAUNCH(k_spd_solve_f64<true>, dim3(n_systems), dim3(threads), lds, st, a, rhs, n, fail);
  else PYZ_LAUNCH(k_spd_solve_f64<false>, dim3(n_systems), dim3(threads), lds, st, a, rhs, n, fail);
}

// ---------------------------------------------------------------- output delta, loss, last layer (FSVI.py:95-98, 111, 123)
struct FsviDelta {
  const float *f;            // act[L - 1]: (k, max_batch, 1)
  long long f_pstride;
  const float *y;            // (rows, 1) targets of the training split
  const int32_t *row_idx;
  const double *alpha;       // (k, n) K_i^-1 f_i
  float *delta_last;         // delta[L - 1], same layout as f
  double *loss_part;         // (k) ll_i
  // the last layer's input: act[L - 2] (k, max_batch, H), or Xp (k, n, F) when the model is one Dense layer
  const float *h;
  long long h_pstride;
  float *delta_prev;         // delta[L - 2] (NULL for a one-layer model)
  const float *theta;        // (k, D) particles
  float *grad;               // (k, D): [dW; db] of the last layer go to w_off
  long long D, w_off;
  int H, b, n, act_last, act_prev;
  float cdat;                // (k / B) (2 / b), float64 rounded once
  double inv_k;
};

// delta_i[r] = ((f - y) cdat [r < b] - (float)(alpha / k)) act'(f): both network terms in one backward pass (A8 step 7).
// One workgroup per particle.  ll_i: thread t sums its rows t, t + 256, ... in float64, then a fixed tree.  With one output
// unit the last layer's backward pass is a rank-one product: delta_prev[r][j] = delta[r] W[j] act'(h[r][j]), and
// dW[j] = sum_r h[r][j] delta[r], db = sum_r delta[r], each a sequential float32 sum over the rows in ascending order.
__global__ void __launch_bounds__(256) k_fsvi_delta(FsviDelta g) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float *f = g.f + i * g.f_pstride;
  float *dl = g.delta_last + i * g.f_pstride;
  double sq = 0.0;
  for (int r = tid; r < g.n; r += 256) {
    const float fr = f[r];
    float data = 0.0f;
    if (r < g.b) {
      const long long row = g.row_idx ? g.row_idx[r] : r;
      const float e = fr - g.y[row];
      data = e * g.cdat;
      sq = fma((double)e, (double)e, sq);
    }
    const float gp = (float)(g.alpha[(long long)i * g.n + r] * g.inv_k);
    dl[r] = (data - gp) * pyz_act_grad(fr, g.act_last);
  }
  red[tid] = sq;
  __syncthreads();                                  // (also: every delta of this particle is written)
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) g.loss_part[i] = red[0] / (double)g.b;
  const int H = g.H;
  const float *hi = g.h + i * g.h_pstride;
  const float *wl = g.theta + i * g.D + g.w_off;     // [W (H); b]
  if (g.delta_prev) {
    float *dp = g.delta_prev + i * g.h_pstride;
    for (long long e = tid; e < (long long)g.n * H; e += 256) {
      const int r = (int)(e / H), j = (int)(e % H);
      dp[e] = (dl[r] * wl[j]) * pyz_act_grad(hi[e], g.act_prev);
    }
  }
  float *go = g.grad + i * g.D + g.w_off;
  for (int j = tid; j <= H; j += 256) {
    float s = 0.0f;
    if (j < H) {
      for (int r = 0; r < g.n; ++r) s = s + hi[(long long)r * H + j] * dl[r];
    } else {
      for (int r = 0; r < g.n; ++r) s = s + dl[r];
    }
    go[j] = s;
  }
}

// ---------------------------------------------------------------- total gradient, Adam, redraw (FSVI.py:115-138, 228-231)
struct FsviUpdate {
  float *mu, *adam_m, *adam_v;   // (D)
  float *particles;              // (k, D): rewritten
  const float *grad;             // (k, D) network gradients of the particles
  const double *stein_sol;       // (k, D) (K_w + 1e-3 I)^-1 rhs: c2 = -solution
  const float *eps;              // optional (k, D); NULL: N(0, 1) from (seed, 9, 4t + 2), element i D + e
  float *stein_out, *grad_out;   // optional (k, D) c2 / (D) g
  const double *loss_part;       // (k)
  const int *fail;               // (2 k) pivot flags of the two solves
  float *loss;
  int *nonfinite;
  long long D;
  int k;
  float inv_k, lr_t;
  uint64_t seed;
  uint32_t t4;
};

// g = sum_i grad_i - (1 / k) sum_i c2_i, both float32 sums in particle order; c2_i is rounded to float32 once.  Keras
// legacy Adam (beta_1 0.9, beta_2 0.999, epsilon 1e-7; lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t) from the host, float64
// rounded once) with the roundings of pyz_svgd_gs_adam; then W_i = mu + eps_i for every particle.
__global__ void __launch_bounds__(256) k_fsvi_update(FsviUpdate g) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < g.D) {
    float gs = 0.0f, cs = 0.0f;
    for (int i = 0; i < g.k; ++i) gs = gs + g.grad[i * g.D + e];
    for (int i = 0; i < g.k; ++i) {
      const float c2 = (float)(-g.stein_sol[i * g.D + e]);
      if (g.stein_out) g.stein_out[i * g.D + e] = c2;
      cs = cs + c2;
    }
    const float gr = gs - g.inv_k * cs;
    if (g.grad_out) g.grad_out[e] = gr;
    float m = g.adam_m[e], v = g.adam_v[e];
    m = m + (gr - m) * (1.0f - 0.9f);
    v = v + (gr * gr - v) * (1.0f - 0.999f);
    const float mu = g.mu[e] - g.lr_t * m / (sqrtf(v) + 1e-7f);
    g.adam_m[e] = m;
    g.adam_v[e] = v;
    g.mu[e] = mu;
    for (int i = 0; i < g.k; ++i) {
      const float z = g.eps ? g.eps[i * g.D + e] : pyz_normal1(g.seed, PYZ_STREAM_FSVI, g.t4 + 2u, (uint64_t)i * g.D + e);
      g.particles[i * g.D + e] = mu + z;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // FSVI.py:123,147: sum_i ll_i / k; a failed factorisation makes it NaN
    double tot = 0.0;
    for (int i = 0; i < g.k; ++i) tot += g.loss_part[i] / (double)g.k;
    bool bad = false;
    for (int i = 0; i < 2 * g.k; ++i) bad = bad || g.fail[i] != 0;
    const float l = bad ? __builtin_nanf("") : (float)tot;
    g.loss[0] = l;
    pyz_note_loss(g.nonfinite, l);
  }
}
