// pyz_pilco.h -- the policy update of Deep-PILCO (Pyesian/dynamics/deep_pilco.py:247-326) as a chain of small kernels.
//
// A rollout moves K particles through H steps.  Particle i has its own draw W_i of the dynamics network; every step
// couples all particles through a mean and a population deviation:
//   a_i = policy(phi, s_i)            the network's output itself (softmax probabilities for a discrete action space)
//   y_i = dynamics(W_i, [s_i, a_i])   last layer linear
//   m = mean_i y_i, sd = sqrt(mean_i (y_i - m)^2),  s'_i = m + sd * eps_i        (:255-261, reparameterised)
//   cost = -mean_i r(s_0,i, 0) - sum over the t with t % freq == 0 of gamma^(t / freq) mean_i r(s_t,i, t)   (:301-316)
// and the gradient of cost with respect to phi goes back through every step (:318).
//
// Decomposition: one workgroup of 256 threads per particle, one launch per step and direction -- the seam between two
// steps is the all-particle mean, and a kernel boundary is the only grid-wide barrier used.  No atomics.
//   k_pilco_set    the scalars of the call (Adam's step size, the per-step cost factors c_t = -gamma^(t / freq) / K, or 0
//                  for a step that is not counted, c_0 = -1 / K) into device memory, so that a captured graph of the
//                  other launches serves every call with the same pointers, H and freq; and the TRANSPOSE of every
//                  kernel (an RBF layer's means too) of phi and of the K draws (32 x 32 tiles through LDS), for the
//                  backward kernels
//   k_pilco_fwd    step t = 1..H: workgroup i stages the K x S raw predictions y of step t - 1 in LDS, column c's thread
//                  sums them in particle order (every workgroup gets the same m and sd), forms s_{t-1,i}, its reward, runs
//                  the policy and its draw of the dynamics with the activations in LDS, and leaves y_t,i and the tape:
//                  s_{t-1,i}, a_{t-1,i}, the hidden activations of both nets, m and sd (written by workgroup 0)
//   k_pilco_tail   s_H,i from y_H, its reward, and the state gradient g_H,i = c_H dr/ds
//   k_pilco_bwd    step t = H..1: workgroup i stages the K x S state gradients g_t and eps_t, forms
//                    d cost / d y_t,i = (sum_j g_j) / K + (y_i - m) / (K sd) * sum_j g_j eps_j      (sums in particle order)
//                  goes back through its dynamics draw to [s, a], through the policy (softmax Jacobian included), adds
//                  the policy's parameter gradient to row i of the (K, D_pol) partial buffer (step H writes it) and
//                  leaves g_{t-1,i} = ds(dynamics) + ds(policy) + c_{t-1} dr/ds(s_{t-1,i})
//   k_pilco_close  grad = the K partial rows summed in particle order, cost = sum_t c_t sum_i r(s_t,i, t) in (t, particle)
//                  order, and one Keras-Adam update of phi when asked
// 2 H + 3 launches, whatever K is.  Every sum has one fixed order, so a call gives the same bits every time, captured or not.
//
// The GEMV: weights are (in, out) row-major.  Forward: a thread per output column reads the kernel coalesced, the input
// vector is an LDS broadcast; layers of at most 128 columns split the reduction over 256 / width thread groups whose
// partial sums are added in group order.  Back-propagation is the same GEMV on the transposed kernels that k_pilco_set
// leaves in the workspace: reading the (in, out) kernel itself by rows needs a cross-lane fold per row, and with
// T = min(64, out) lanes per row and an xor butterfly (ds_bpermute) k_pilco_bwd took 122 us per step at the example
// shape (9 -> 512 -> 256 -> 6, K = 32) against 19 us for k_pilco_fwd; the transposition costs one pass over the weights
// per policy update.  Loads are unconditional (indices clamped): a load under a branch is waited for at the branch's join.
//
// The RBF layer (deep_pilco.py:28-51), a hidden layer of the policy only: h[n] = exp(-gamma sum_k (x[k] - mean[k][n])^2),
// `mean` (in, units) row-major at the layer's offset of phi, no bias (the layer takes in * units floats), gamma a
// constant of the layer.  Forward: pilco_rbf, the access pattern of pilco_gemv.  Backward, with delta the gradient with
// respect to h and e[n] = 2 gamma delta[n] h[n]:  d mean[k][n] = e[n] (x[k] - mean[k][n]),  d x[k] = -sum_n e[n] (x[k] -
// mean[k][n]), the latter one pass over the transposed means of k_pilco_set (pilco_rbf_dx); the h factor is taken there,
// so no activation gradient follows an RBF layer.  The branch on the layer kind is the same in every thread of a launch.
//
// k_pilco_act is the policy alone for N given states, a workgroup per row, through the same pilco_policy as k_pilco_fwd.
//
// Limits (checked on the host, before any launch): 2 <= K <= 256, 1 <= S, 1 <= A, S + A <= 64, layer widths <= 512, at most
// PILCO_MAX_LAYERS layers per net, the policy's last layer Dense, H <= max_horizon <= 4096.
#pragma once

#include "pyz_common.h"
#include "pyz_gemm.h"

#define PILCO_MAX_LAYERS 8
#define PILCO_MAX_WIDTH 512
#define PILCO_MAX_K 256
#define PILCO_MAX_IN 64
#define PILCO_MAX_H 4096
#ifndef PILCO_THREADS
#define PILCO_THREADS 256   // of the two step kernels (a power of two)
#endif

struct PilcoNet {
  int L;
  int dims[PILCO_MAX_LAYERS + 1];
  int acts[PILCO_MAX_LAYERS];    // (linear for an RBF layer)
  int w_off[PILCO_MAX_LAYERS];   // layer l's kernel (a Dense layer's bias follows) in the flat vector
  int kind[PILCO_MAX_LAYERS];    // PYZ_PILCO_DENSE: (in + 1) * out floats; PYZ_PILCO_RBF: the means, in * out floats
  float gamma[PILCO_MAX_LAYERS]; // of an RBF layer
};

struct PilcoCtl {
  float lr_t;     // lr sqrt(1 - b2^t) / (1 - b1^t)
  int adam_on;    // 0: gradient only
};

struct PilcoArgs {
  PilcoNet pol, dyn;
  int K, S, A, H, reward;
  int maxw;             // widest vector of either net
  int tw, tw_pol;       // tape floats per (step, particle); those of the policy's hidden layers come first
  int pw;               // s, the policy's hidden activations and a, in a row
  long long Dp, Dd;
  const float *phi, *W, *s0, *eps;
  float *phiT, *WT;     // (Dp), (K, Dd): every kernel (in, out) transposed to (out, in) at its own offset; biases unused
  float *y;             // (H, K, S) raw predictions, y_t at row t - 1
  float *st;            // (H + 1, K, S)
  float *ac;            // (H, K, A)
  float *tape;          // (H, K, tw)
  float *msd;           // (H, 2, S) m_t, sd_t at row t - 1
  float *g;             // (2, K, S) state gradients of step t at row t & 1
  float *rew;           // (H + 1, K)
  float *coef;          // (H + 1)
  float *part;          // (K, Dp)
  const PilcoCtl *ctl;
  float *m, *v, *phi_out, *cost, *grad;
  int t;
};

// LDS bytes of the two step kernels and of k_pilco_act
static inline size_t pilco_fwd_lds(int K, int S, int maxw) { return sizeof(float) * ((size_t)K * S + PILCO_MAX_IN + 2 * (size_t)maxw + PILCO_THREADS); }
static inline size_t pilco_act_lds(int maxw) { return sizeof(float) * (PILCO_MAX_IN + 2 * (size_t)maxw + PILCO_THREADS); }
static inline size_t pilco_bwd_lds(int K, int S, int maxw, int pw) {
  return sizeof(float) * (2 * (size_t)K * S + PILCO_MAX_IN + (size_t)pw + 2 * (size_t)maxw + PILCO_THREADS);
}

__device__ __forceinline__ float pilco_reward(int id, const float *s, float t) {
  if (id == PYZ_REWARD_CART) return -s[2] - s[3] * s[2] + t * (-s[2] * s[2] + 0.2095f * 0.2095f);
  return 4.0f - 3.0f * s[0] - (s[0] * s[2] - s[1] * s[3]) + s[4] * s[4];
}

// d r / d s_c
__device__ __forceinline__ float pilco_reward_grad(int id, const float *s, float t, int c) {
  if (id == PYZ_REWARD_CART) {
    if (c == 2) return -1.0f - s[3] - 2.0f * t * s[2];
    if (c == 3) return -s[2];
    return 0.0f;
  }
  switch (c) {
    case 0: return -3.0f - s[2];
    case 1: return s[3];
    case 2: return -s[0];
    case 3: return s[1];
    case 4: return 2.0f * s[4];
    default: return 0.0f;
  }
}

// out[n] = b[n] + sum_k in[k] w[k][n] for n < N, w (Kin, N) row-major (in, out, part: LDS; out != in; bias may be null:
// 0).  Ends with a barrier.
__device__ __forceinline__ void pilco_gemv(const float *__restrict__ w, const float *__restrict__ bias, int Kin, int N,
                                           const float *in, float *out, float *part) {
  const int tid = threadIdx.x;
  if (N > PILCO_THREADS / 2) {
    for (int n0 = 0; n0 < N; n0 += PILCO_THREADS) {
      const int n = min(n0 + tid, N - 1);
      const float *col = w + n;
      float acc = bias ? bias[n] : 0.0f;
#pragma unroll 16
      for (int k = 0; k < Kin; ++k) acc = fmaf(in[k], col[(long long)k * N], acc);
      if (n0 + tid < N) out[n0 + tid] = acc;
    }
  } else {
    int NP = 1;
    while (NP < N) NP <<= 1;
    const int G = PILCO_THREADS / NP, gi = tid / NP, n = tid % NP;
    const int len = (Kin + G - 1) / G;
    const int k0 = min(gi * len, Kin), k1 = min(k0 + len, Kin);
    const float *col = w + min(n, N - 1);
    float acc = 0.0f;
#pragma unroll 16
    for (int k = k0; k < k1; ++k) acc = fmaf(in[k], col[(long long)k * N], acc);
    part[tid] = acc;                                  // tid = gi * NP + n
    __syncthreads();
    if (tid < N) {
      float s = bias ? bias[tid] : 0.0f;
      for (int q = 0; q < G; ++q) s += part[q * NP + tid];
      out[tid] = s;
    }
  }
  __syncthreads();
}

// out[n] = exp(-gamma sum_k (in[k] - w[k][n])^2) for n < N, w (Kin, N) row-major: pilco_gemv's walk over the means, its
// split over thread groups and its order of the partial sums.  Ends with a barrier.
__device__ __forceinline__ void pilco_rbf(const float *__restrict__ w, float gamma, int Kin, int N, const float *in, float *out,
                                          float *part) {
  const int tid = threadIdx.x;
  if (N > PILCO_THREADS / 2) {
    for (int n0 = 0; n0 < N; n0 += PILCO_THREADS) {
      const int n = min(n0 + tid, N - 1);
      const float *col = w + n;
      float acc = 0.0f;
#pragma unroll 16
      for (int k = 0; k < Kin; ++k) {
        const float d = in[k] - col[(long long)k * N];
        acc = fmaf(d, d, acc);
      }
      if (n0 + tid < N) out[n0 + tid] = expf(-gamma * acc);
    }
  } else {
    int NP = 1;
    while (NP < N) NP <<= 1;
    const int G = PILCO_THREADS / NP, gi = tid / NP, n = tid % NP;
    const int len = (Kin + G - 1) / G;
    const int k0 = min(gi * len, Kin), k1 = min(k0 + len, Kin);
    const float *col = w + min(n, N - 1);
    float acc = 0.0f;
#pragma unroll 16
    for (int k = k0; k < k1; ++k) {
      const float d = in[k] - col[(long long)k * N];
      acc = fmaf(d, d, acc);
    }
    part[tid] = acc;                                  // tid = gi * NP + n
    __syncthreads();
    if (tid < N) {
      float s = 0.0f;
      for (int q = 0; q < G; ++q) s += part[q * NP + tid];
      out[tid] = expf(-gamma * s);
    }
  }
  __syncthreads();
}

// out[k] = -sum_n e[n] (x[k] - wT[n][k]) for k < Kin, wT (N, Kin) row-major: the transposed means (e, x, out, part: LDS; out
// is neither e nor x).  A thread per k reads wT coalesced; the split and the order of the sums are pilco_gemv's.  Ends with
// a barrier.
__device__ __forceinline__ void pilco_rbf_dx(const float *__restrict__ wT, int N, int Kin, const float *e, const float *x,
                                             float *out, float *part) {
  const int tid = threadIdx.x;
  if (Kin > PILCO_THREADS / 2) {
    for (int c0 = 0; c0 < Kin; c0 += PILCO_THREADS) {
      const int k = min(c0 + tid, Kin - 1);
      const float *col = wT + k;
      const float xk = x[k];
      float acc = 0.0f;
#pragma unroll 16
      for (int n = 0; n < N; ++n) acc = fmaf(e[n], xk - col[(long long)n * Kin], acc);
      if (c0 + tid < Kin) out[c0 + tid] = -acc;
    }
  } else {
    int KP = 1;
    while (KP < Kin) KP <<= 1;
    const int G = PILCO_THREADS / KP, gi = tid / KP, k = min(tid % KP, Kin - 1);
    const int len = (N + G - 1) / G;
    const int n0 = min(gi * len, N), n1 = min(n0 + len, N);
    const float *col = wT + k;
    const float xk = x[k];
    float acc = 0.0f;
#pragma unroll 16
    for (int n = n0; n < n1; ++n) acc = fmaf(e[n], xk - col[(long long)n * Kin], acc);
    part[tid] = acc;                                  // tid = gi * KP + (tid % KP)
    __syncthreads();
    if (tid < Kin) {
      float s = 0.0f;
      for (int q = 0; q < G; ++q) s += part[q * KP + tid];
      out[tid] = -s;
    }
  }
  __syncthreads();
}

// s_u,i (u = 0..H) into sout[0 .. S) (LDS) and st, its reward into rew; u >= 1: m_u and sd_u from the staged y_u, which
// workgroup 0 also leaves in msd.  Ends with a barrier.
__device__ __forceinline__ void pilco_state(const PilcoArgs &g, int u, float *yl, float *sout) {
  const int tid = threadIdx.x, i = blockIdx.x, K = g.K, S = g.S, KS = K * S;
  const int c = min(tid, S - 1);
  if (u == 0) {                                                                  // (uniform)
    const float s = g.s0[i * S + c];
    if (tid < S) {
      sout[tid] = s;
      g.st[i * S + tid] = s;
    }
  } else {
    const float e = g.eps[(long long)(u - 1) * KS + i * S + c];
    const float *ysrc = g.y + (long long)(u - 1) * KS;
    for (int q = tid; q < KS; q += PILCO_THREADS) yl[q] = ysrc[q];
    __syncthreads();
    if (tid < S) {
      float sum = 0.0f;
#pragma unroll 8
      for (int j = 0; j < K; ++j) sum += yl[j * S + tid];
      const float m = sum / (float)K;
      float sq = 0.0f;
#pragma unroll 8
      for (int j = 0; j < K; ++j) {
        const float d = yl[j * S + tid] - m;
        sq = fmaf(d, d, sq);
      }
      const float sd = sqrtf(sq / (float)K);
      const float s = fmaf(sd, e, m);
      sout[tid] = s;
      g.st[(long long)u * KS + i * S + tid] = s;
      if (i == 0) {
        g.msd[(long long)(u - 1) * 2 * S + tid] = m;
        g.msd[(long long)(u - 1) * 2 * S + S + tid] = sd;
      }
    }
  }
  __syncthreads();
  if (tid == 0) g.rew[(long long)u * K + i] = pilco_reward(g.reward, sout, (float)u);
}

// The policy: xin[0 .. S) -> xin[S .. S + A) (LDS) and arow[0 .. A); TAPE: the hidden activations, in layer order, to
// tape[0 .. tw_pol).  Ends with a barrier.
template <bool TAPE>
__device__ __forceinline__ void pilco_policy(const PilcoArgs &g, float *xin, float *bufA, float *bufB, float *part, float *tape,
                                             float *arow) {
  const int tid = threadIdx.x, S = g.S;
  const float *in = xin;
  float *out = bufA;
  for (int l = 0; l < g.pol.L; ++l) {
    const int Kin = g.pol.dims[l], N = g.pol.dims[l + 1], act = g.pol.acts[l];
    const float *w = g.phi + g.pol.w_off[l];
    if (g.pol.kind[l] == PYZ_PILCO_RBF) pilco_rbf(w, g.pol.gamma[l], Kin, N, in, out, part);     // (uniform)
    else pilco_gemv(w, w + Kin * N, Kin, N, in, out, part);
    if (l + 1 < g.pol.L) {
      for (int n = tid; n < N; n += PILCO_THREADS) {
        const float h = pyz_act(out[n], act);
        out[n] = h;
        if (TAPE) tape[n] = h;
      }
      if (TAPE) tape += N;
      in = out;
      out = out == bufA ? bufB : bufA;
    } else {
      if (tid < N) {
        float a;
        if (act == PYZ_ACT_SOFTMAX) {
          float mx = out[0];
          for (int k = 1; k < N; ++k) mx = fmaxf(mx, out[k]);
          float se = 0.0f;
          for (int k = 0; k < N; ++k) se += expf(out[k] - mx);
          a = expf(out[tid] - mx) / se;
        } else {
          a = pyz_act(out[tid], act);
        }
        xin[S + tid] = a;
        arow[tid] = a;
      }
    }
    __syncthreads();
  }
}

// grid (x, K + 2): rows y < K transpose draw y's kernels, row K the policy's, row K + 1 writes the scalars and c_t
__global__ void __launch_bounds__(256) k_pilco_set(PilcoArgs g, PilcoCtl *ctl, int freq, double gamma, float lr_t, int adam_on) {
  __shared__ float tile[32][33];
  const int tid = threadIdx.x, y = blockIdx.y, K = g.K;
  if (y == K + 1) {
    const int t = blockIdx.x * 256 + tid;
    if (t == 0) {
      ctl->lr_t = lr_t;
      ctl->adam_on = adam_on;
    }
    if (t > g.H) return;
    double c = 0.0;
    if (t == 0) c = -1.0 / K;
    else if (t % freq == 0) c = -pow(gamma, (double)(t / freq)) / K;
    g.coef[t] = (float)c;
    return;
  }
  const bool pol = y == K;
  const int L = pol ? g.pol.L : g.dyn.L;
  const float *src = pol ? g.phi : g.W + (long long)y * g.Dd;
  float *dst = pol ? g.phiT : g.WT + (long long)y * g.Dd;
  int b = blockIdx.x, l = 0, Kin = 0, N = 0, off = 0, tc = 1;
  for (; l < L; ++l) {                                   // which layer's tile this block is (uniform)
    Kin = pol ? g.pol.dims[l] : g.dyn.dims[l];
    N = pol ? g.pol.dims[l + 1] : g.dyn.dims[l + 1];
    off = pol ? g.pol.w_off[l] : g.dyn.w_off[l];
    tc = (N + 31) / 32;
    const int tiles = ((Kin + 31) / 32) * tc;
    if (b < tiles) break;
    b -= tiles;
  }
  if (l == L) return;
  const int r0 = (b / tc) * 32, c0 = (b % tc) * 32, tx = tid & 31, ty = tid >> 5;
#pragma unroll
  for (int j = 0; j < 32; j += 8) {
    const int r = r0 + ty + j, c = c0 + tx;
    if (r < Kin && c < N) tile[ty + j][tx] = src[off + r * N + c];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 32; j += 8) {
    const int c = c0 + ty + j, r = r0 + tx;
    if (c < N && r < Kin) dst[off + c * Kin + r] = tile[tx][ty + j];
  }
}

__global__ void __launch_bounds__(PILCO_THREADS) k_pilco_fwd(PilcoArgs g) {
  extern __shared__ __attribute__((aligned(16))) float pilco_lds[];
  const int tid = threadIdx.x, i = blockIdx.x, K = g.K, S = g.S, A = g.A, t = g.t;
  float *yl = pilco_lds, *xin = yl + K * S, *bufA = xin + PILCO_MAX_IN, *bufB = bufA + g.maxw, *part = bufB + g.maxw;
  pilco_state(g, t - 1, yl, xin);

  float *tape = g.tape + ((long long)(t - 1) * K + i) * g.tw;
  pilco_policy<true>(g, xin, bufA, bufB, part, tape, g.ac + ((long long)(t - 1) * K + i) * A);
  tape += g.tw_pol;
  // this particle's draw of the dynamics: xin[0 .. S + A) -> y_t,i
  {
    const float *wd = g.W + (long long)i * g.Dd;
    const float *in = xin;
    float *out = bufA;
    for (int l = 0; l < g.dyn.L; ++l) {
      const int Kin = g.dyn.dims[l], N = g.dyn.dims[l + 1], act = g.dyn.acts[l];
      pilco_gemv(wd + g.dyn.w_off[l], wd + g.dyn.w_off[l] + Kin * N, Kin, N, in, out, part);
      if (l + 1 < g.dyn.L) {
        for (int n = tid; n < N; n += PILCO_THREADS) {
          const float h = pyz_act(out[n], act);
          out[n] = h;
          tape[n] = h;
        }
        tape += N;
        in = out;
        out = out == bufA ? bufB : bufA;
        __syncthreads();
      } else if (tid < N) {
        g.y[((long long)(t - 1) * K + i) * S + tid] = out[tid];
      }
    }
  }
}

// grid (rows): workgroup i is the policy of k_pilco_fwd on row i of states (rows, S), into row i of actions (rows, A)
__global__ void __launch_bounds__(PILCO_THREADS) k_pilco_act(PilcoArgs g, const float *__restrict__ states, float *actions) {
  extern __shared__ __attribute__((aligned(16))) float pilco_lds[];
  const int tid = threadIdx.x, S = g.S;
  const long long i = blockIdx.x;
  float *xin = pilco_lds, *bufA = xin + PILCO_MAX_IN, *bufB = bufA + g.maxw, *part = bufB + g.maxw;
  const float s = states[i * S + min(tid, S - 1)];
  if (tid < S) xin[tid] = s;
  __syncthreads();
  pilco_policy<false>(g, xin, bufA, bufB, part, nullptr, actions + i * g.A);
}

__global__ void __launch_bounds__(PILCO_THREADS) k_pilco_tail(PilcoArgs g) {
  extern __shared__ __attribute__((aligned(16))) float pilco_lds[];
  const int tid = threadIdx.x, i = blockIdx.x, K = g.K, S = g.S, H = g.H;
  float *yl = pilco_lds, *xin = yl + K * S;
  pilco_state(g, H, yl, xin);
  if (tid < S) g.g[((long long)(H & 1) * K + i) * S + tid] = g.coef[H] * pilco_reward_grad(g.reward, xin, (float)H, tid);
}

__global__ void __launch_bounds__(PILCO_THREADS) k_pilco_bwd(PilcoArgs g) {
  extern __shared__ __attribute__((aligned(16))) float pilco_lds[];
  const int tid = threadIdx.x, i = blockIdx.x, K = g.K, S = g.S, A = g.A, t = g.t, KS = K * S;
  float *gl = pilco_lds, *ge = gl + KS, *dsd = ge + KS, *pact = dsd + PILCO_MAX_IN, *dA = pact + g.pw, *dB = dA + g.maxw,
        *part = dB + g.maxw;

  {  // d cost / d y_t,i -> dA[0 .. S)
    const float *gsrc = g.g + (long long)(t & 1) * KS, *esrc = g.eps + (long long)(t - 1) * KS;
    const int c = min(tid, S - 1);
    const float m = g.msd[(long long)(t - 1) * 2 * S + c], sd = g.msd[(long long)(t - 1) * 2 * S + S + c];
    const float yi = g.y[((long long)(t - 1) * K + i) * S + c];
    for (int q = tid; q < KS; q += PILCO_THREADS) {
      const float gv = gsrc[q];
      gl[q] = gv;
      ge[q] = gv * esrc[q];
    }
    // s_{t-1,i}, the policy's hidden activations and a_{t-1,i} in a row
    const float *tape = g.tape + ((long long)(t - 1) * K + i) * g.tw;
    const int nh = g.tw_pol;
    for (int q = tid; q < g.pw; q += PILCO_THREADS) {
      float v;
      if (q < S) v = g.st[((long long)(t - 1) * K + i) * S + q];
      else if (q < S + nh) v = tape[q - S];
      else v = g.ac[((long long)(t - 1) * K + i) * A + (q - S - nh)];
      pact[q] = v;
    }
    __syncthreads();
    if (tid < S) {
      float g1 = 0.0f, g2 = 0.0f;
#pragma unroll 8
      for (int j = 0; j < K; ++j) {
        g1 += gl[j * S + tid];
        g2 += ge[j * S + tid];
      }
      dA[tid] = g1 / (float)K + (yi - m) / ((float)K * sd) * g2;
    }
    __syncthreads();
  }

  float *delta = dA, *other = dB;
  {  // back through the dynamics draw: delta (S) -> d [s, a]
    const float *wt = g.WT + (long long)i * g.Dd;
    const float *tape = g.tape + ((long long)(t - 1) * K + i) * g.tw + g.tw;   // one past the last dynamics hidden layer
    for (int l = g.dyn.L - 1; l >= 0; --l) {
      const int Kin = g.dyn.dims[l], N = g.dyn.dims[l + 1];
      pilco_gemv(wt + g.dyn.w_off[l], nullptr, N, Kin, delta, other, part);
      if (l > 0) {
        tape -= Kin;                                                             // the output of layer l - 1
        const int act = g.dyn.acts[l - 1];
        for (int k = tid; k < Kin; k += PILCO_THREADS) other[k] *= pyz_act_grad(tape[k], act);
        __syncthreads();
      }
      float *sw = delta;
      delta = other;
      other = sw;
    }
  }
  // delta = d [s, a]: keep ds, turn da into the policy's output delta
  {
    const int Lp = g.pol.L, act = g.pol.acts[Lp - 1];
    const float *a = pact + g.pw - A;
    float dz = 0.0f;
    if (tid < A) {
      const float da = delta[S + tid];
      if (act == PYZ_ACT_SOFTMAX) {
        float dot = 0.0f;
        for (int k = 0; k < A; ++k) dot = fmaf(delta[S + k], a[k], dot);
        dz = a[tid] * (da - dot);
      } else {
        dz = da * pyz_act_grad(a[tid], act);
      }
    }
    if (tid < S) dsd[tid] = delta[tid];
    __syncthreads();
    if (tid < A) delta[tid] = dz;
    __syncthreads();
  }
  {  // back through the policy: parameter gradients into row i of part, ds into `delta`
    float *prow = g.part + (long long)i * g.Dp;
    const bool first = t == g.H;
    const float *in = pact + g.pw - A;            // walks back over the layer inputs
    for (int l = g.pol.L - 1; l >= 0; --l) {
      const int Kin = g.pol.dims[l], N = g.pol.dims[l + 1];
      in -= Kin;
      float *pw = prow + g.pol.w_off[l];
      if (g.pol.kind[l] == PYZ_PILCO_RBF) {         // (uniform)
        const float *h = in + Kin, *mean = g.phi + g.pol.w_off[l];   // the layer's output follows its input in pact
        const float g2 = 2.0f * g.pol.gamma[l];
        for (int n = tid; n < N; n += PILCO_THREADS) delta[n] = g2 * delta[n] * h[n];          // delta -> e
        __syncthreads();
        const int nw = Kin * N;                     // the means: no bias row
        for (int e = tid; e < nw; e += PILCO_THREADS) {
          const int k = e / N, n = e - k * N;
          const float d = in[k] - mean[e];
          const float old = first ? 0.0f : pw[e];
          pw[e] = fmaf(delta[n], d, old);
        }
        pilco_rbf_dx(g.phiT + g.pol.w_off[l], N, Kin, delta, in, other, part);
      } else {
        const int nw = (Kin + 1) * N;               // kernel, then bias (input 1)
        for (int e = tid; e < nw; e += PILCO_THREADS) {
          const int k = e / N, n = e - k * N;
          const float x = k < Kin ? in[k] : 1.0f;
          const float old = first ? 0.0f : pw[e];
          pw[e] = fmaf(x, delta[n], old);
        }
        pilco_gemv(g.phiT + g.pol.w_off[l], nullptr, N, Kin, delta, other, part);
      }
      if (l > 0 && g.pol.kind[l - 1] == PYZ_PILCO_DENSE) {     // an RBF layer's h factor is taken in its own step
        const int act = g.pol.acts[l - 1];
        for (int k = tid; k < Kin; k += PILCO_THREADS) other[k] *= pyz_act_grad(in[k], act);
        __syncthreads();
      }
      float *sw = delta;
      delta = other;
      other = sw;
    }
  }
  if (t > 1 && tid < S)
    g.g[((long long)((t - 1) & 1) * K + i) * S + tid] =
        dsd[tid] + delta[tid] + g.coef[t - 1] * pilco_reward_grad(g.reward, pact, (float)(t - 1), tid);
}

__global__ void __launch_bounds__(256) k_pilco_close(PilcoArgs g) {
  __shared__ float cs[256];
  const int tid = threadIdx.x, K = g.K;
  const long long e = (long long)blockIdx.x * 256 + tid;
  if (e < g.Dp) {
    float s = 0.0f;
    for (int j = 0; j < K; ++j) s += g.part[(long long)j * g.Dp + e];
    g.grad[e] = s;
    if (g.ctl->adam_on) {
      float m = g.m[e], v = g.v[e];
      m += (s - m) * 0.1f;                 // 1 - beta evaluated in float64 and rounded once, as Keras does
      v += (s * s - v) * 0.001f;
      g.m[e] = m;
      g.v[e] = v;
      g.phi_out[e] = g.phi_out[e] - g.ctl->lr_t * m / (sqrtf(v) + 1e-7f);
    }
  }
  if (blockIdx.x != 0) return;
  float acc = 0.0f;
  for (int u0 = 0; u0 <= g.H; u0 += 256) {   // (uniform)
    const int u = u0 + tid;
    float s = 0.0f;
    if (u <= g.H) {
      const float c = g.coef[u];
      if (c != 0.0f) {
        for (int j = 0; j < K; ++j) s += g.rew[(long long)u * K + j];
        s *= c;
      }
    }
    cs[tid] = s;
    __syncthreads();
    if (tid == 0) {
      const int n = min(256, g.H + 1 - u0);
      for (int q = 0; q < n; ++q) acc += cs[q];
    }
    __syncthreads();
  }
  if (tid == 0) g.cost[0] = acc;
}
