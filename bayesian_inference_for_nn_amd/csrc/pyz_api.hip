// pyz_api.hip -- extern "C" entry points declared in include/pyz.h.
// Host-side orchestration only: shape checks, workspace, kernel launches.

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "pyz_common.h"
#include "pyz_conv.h"
#include "pyz_corrupt.h"
#include "pyz_fsvi.h"
#include "pyz_fused.h"
#include "pyz_gemm.h"
#include "pyz_gemm_ring.h"
#include "pyz_hmc_fused.h"
#include "pyz_hmc_multi.h"
#include "pyz_input_grad.h"
#include "pyz_pilco.h"
#include "pyz_kernels.h"
#include "pyz_predict_moments.h"
#include "pyz_surface.h"
#include "pyz_rng.h"
#include "pyz_sgld_chains.h"
#include "pyz_sgld_lanes.h"
#include "pyz_bbb_lanes.h"
#include "pyz_members.h"

namespace {

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

void drop_graphs(pyz_mlp *m);

// Grows a lazily sized buffer of the plan.  A buffer that MOVES takes every captured graph of the plan with it: the graphs
// bake in the plan's pointers (m->grad in the unfused chained SGLD step, grad2, part2, hm_buf, ...), and a replay would read
// and write what was just freed.  The keys of the caches still mix the pointers they know of; dropping here covers the ones
// they do not, for every buffer that goes through this function.  Growth is rare (a call with more particles than any
// before it) and never happens inside a capture: every run sizes its buffers before it captures.  The first allocation
// (nothing to move) drops nothing.
int ensure_bytes(void **ptr, size_t *cap, size_t need, pyz_mlp *m) {
  if (*cap >= need) return PYZ_OK;
  if (*ptr) {
    PYZ_HIP(hipDeviceSynchronize());   // a graph launched on any stream may still use the buffer, and is destroyed below
    PYZ_HIP(hipFree(*ptr));
    drop_graphs(m);
  }
  *ptr = nullptr;
  *cap = 0;
  PYZ_HIP(hipMalloc(ptr, need));
  m->ws_bytes += need;
  *cap = need;
  return PYZ_OK;
}

struct Extra {  // lazily sized buffers kept beside the plan
  size_t grad_cap = 0, grad2_cap = 0, qsave_cap = 0, part_cap = 0, part2_cap = 0, scal_cap = 0;
  void *hm_buf = nullptr;  // k_hmc_multi: state / slab ping-pong buffers
  size_t hm_cap = 0;
  void *hm_res_buf = nullptr;  // k_hmc_resident: per-chain epochs and the granule rows
  size_t hm_res_cap = 0;
  void *fwd_part = nullptr;    // k_dense_fwd_ring with a split reduction: (k_split, max_batch, width) raw partial sums
  size_t fwd_part_cap = 0;
  void *gs_res_buf = nullptr;  // k_svgd_gs_resident: epoch, fail flag, granules of the partials and of the kernel row
  size_t gs_res_cap = 0;
  PyzGraphCache<1> hm_graphs;  // the launch sequence of one sliced HMC proposal
  double *part2 = nullptr;
  // per-run tables go up through two pinned buffers used in turn (an event each: rewritten only once its copy has left)
  void *tab_host = nullptr;
  size_t tab_host_cap = 0;  // bytes per buffer
  hipEvent_t tab_ev[2] = {};
  unsigned long long tab_count = 0;
  // pyz_adam_run: the bias-correction pairs beside tab_bs / tab_lr
  float2 *tab_bc = nullptr;
  int tab_bc_cap = 0;
  // ... and these runs' own graph cache (a graph of these runs bakes in the launch geometry of every step: the batch size
  // of its chunk, its signature).  A graph holds steps of one batch size and starts on one StepCtl slot, and a quiet
  // train() cuts its stretches of equal batches wherever its resident chunks end: stretch lengths 1 .. batches per epoch in
  // two parities, plus the ragged batch.  AR_GRAPHS slots keep all of them for epochs of up to ~14 batches; longer epochs
  // mostly see full chunks.  Its captures: graphs the last call had to capture (pyz_adam_run_info).
  static constexpr int AR_GRAPHS = 32;
  PyzGraphCache<AR_GRAPHS> adam_graphs;
  // per-proposal HMC scalars (uniforms + HmcCall) go up through a ring of pinned slots: a copy from pageable
  // memory would make every pyz_hmc_step wait for the stream, i.e. serialise the host with the device
  static constexpr int UP_SLOTS = 64;
  unsigned char *up_host = nullptr;
  size_t up_slot_bytes = 0;
  hipEvent_t up_ev[UP_SLOTS] = {};
  unsigned long long up_count = 0;
  // pyz_hmc_run: the proposals of a run take their uniforms and HmcCall from the device (k_hmc_feed), not from the ring
  bool hm_fed = false;           // set around the run's calls of pyz_hmc_step: no upload, no graph of its own
  int hm_path = 0;               // what the last pyz_hmc_step launched: 0 generic, 1 one workgroup, 2 sliced, 3 resident
  unsigned long long hm_sig = 0; // ... and, for the sliced forms, everything its launches bake in
  void *hr_buf = nullptr;        // HmcRunCtl, the count snapshot and the (max_p, 8) statistics of the proposal in flight
  float *hr_tab = nullptr;       // the uniform table of the call
  size_t hr_tab_cap = 0;         // floats
  unsigned char *hr_host = nullptr;  // ... goes up through two pinned buffers used in turn (as tab_host does)
  size_t hr_host_cap = 0;        // bytes per buffer
  hipEvent_t hr_ev[2] = {};
  unsigned long long hr_count = 0;
  // slot 0 = a chunk of proposals, the others = remainders by exact length (LRU); its captures: those of the last pyz_hmc_run
  PyzGraphCache<PYZ_GRAPH_CHUNKS> hmc_run_graphs;
  void *fsvi_buf = nullptr;      // pyz_fsvi_step: Xp, the two float64 systems, their right-hand sides, flags and loss partials
  size_t fsvi_cap = 0;
};

}  // namespace

// The opaque handle = plan + lazily grown buffers.
struct pyz_mlp_full : pyz_mlp {
  Extra x;
};

// A conv net: a stem (pyz_conv.h) in front of a Dense tail.
struct StemOp {
  int kind = 0;
  int H = 0, W = 0, C = 0;         // input map
  int OH = 0, OW = 0, N = 0;       // output map (a pool keeps C)
  int kh = 0, kw = 0, pt = 0, pl = 0, act = 0;   // conv: kernel, top / left padding, activation; pool: kh x kw windows
  int K = 0, KT = 0;               // conv: taps, and table entries (taps + bias, padded to even)
  long long w_off = 0;
  int2 *ktab = nullptr;
  float *out = nullptr, *delta = nullptr;   // (max_p, max_batch, OH * OW * N) each
  int32_t *win = nullptr;          // pool: the winners
  long long size() const { return (long long)OH * OW * N; }
};

struct pyz_stem {
  int n_ops = 0;
  StemOp op[PYZ_STEM_MAX_OPS];
  int in_h = 0, in_w = 0, in_c = 0, max_batch = 0, max_p = 0;
  long long D = 0, F = 0;
  size_t ws_bytes = 0;
  float *part = nullptr;           // partial tiles of the weight gradients (stem_part_bytes)
  bool forwarded = false;          // a forward has left every op's output in the workspace
};

namespace {

inline pyz_mlp_full *full(pyz_mlp *m) { return static_cast<pyz_mlp_full *>(m); }

void drop_graphs(pyz_mlp *m) {
  m->graphs.drop();
  full(m)->x.hm_graphs.drop();
  full(m)->x.hmc_run_graphs.drop();
  full(m)->x.adam_graphs.drop();
}

int need_grad(pyz_mlp *m, int P) {
  m->grad_owner = 2;   // (pyz_svgd_gradients sets 1 after this call)
  return ensure_bytes((void **)&m->grad, &full(m)->x.grad_cap, sizeof(float) * (size_t)P * m->D + 64, m);
}
int need_grad2(pyz_mlp *m, int P) {
  return ensure_bytes((void **)&m->grad2, &full(m)->x.grad2_cap, sizeof(float) * (size_t)P * m->D + 64, m);
}
int need_qsave(pyz_mlp *m, int P) {
  return ensure_bytes((void **)&m->qsave, &full(m)->x.qsave_cap, sizeof(float) * (size_t)P * m->D + 64, m);
}
int need_part(pyz_mlp *m, size_t n_doubles) {
  return ensure_bytes((void **)&m->part, &full(m)->x.part_cap, sizeof(double) * n_doubles, m);
}
int need_part2(pyz_mlp *m, size_t n_doubles, bool keep_kernel_matrix = false) {
  if (!keep_kernel_matrix) m->km_valid = false;   // the float64 scratch is about to be rewritten
  return ensure_bytes((void **)&full(m)->x.part2, &full(m)->x.part2_cap, sizeof(double) * n_doubles, m);
}

int check_call(const pyz_mlp *m, int P, int batch) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (batch <= 0 || batch > m->max_batch)
    return pyz_fail(PYZ_E_SHAPE, "batch %d outside [1, %d] of the plan", batch, m->max_batch);
  if (P <= 0 || P > m->max_p)
    return pyz_fail(PYZ_E_SHAPE, "particle count %d outside [1, %d] of the plan", P, m->max_p);
  return PYZ_OK;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int set_ctl(pyz_mlp *m, int slot, int batch, float lr, long long n, long long row_off, int i, hipStream_t st,
            int slot0 = 0, int n_run = 0) {
  m->pend_on = false;
  PYZ_LAUNCH(k_set_ctl, dim3(1), dim3(1), 0, st, m->ctl + slot, batch, lr, n, row_off, i, slot0, n_run);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// eager steps: no launch for the scalars -- the first kernel of the fused step carries them (pyz_ctl_first)
void set_ctl_lazy(pyz_mlp *m, int batch, float lr, long long n) {
  m->pend = StepCtl{};
  m->pend.batch = batch;
  m->pend.lr = lr;
  m->pend.n = n;
  m->pend_on = true;
}

void flush_ctl(pyz_mlp *m, hipStream_t st) {
  if (!m->pend_on) return;
  m->pend_on = false;
  PYZ_LAUNCH(k_set_ctl, dim3(1), dim3(1), 0, st, m->ctl, m->pend.batch, m->pend.lr, m->pend.n, m->pend.row_off, m->pend.i,
                     m->pend.slot0, 0);
}

// arguments of the forward pass of layer l (activations land in m->act[l])
DenseArgs forward_args(pyz_mlp *m, int l, const float *theta, long long theta_ps, const float *x, const int32_t *row_idx,
                       const StepCtl *ctl, float *gather_out) {
  DenseArgs g{};
  g.K = m->dims[l];
  g.N = m->dims[l + 1];
  if (l == 0) {
    g.in = x;
    g.in_pstride = 0;
    g.row_idx = row_idx;
    g.gather_out = row_idx ? gather_out : nullptr;
  } else {
    g.in = m->act[l - 1];
    g.in_pstride = (long long)m->max_batch * g.K;
    g.row_idx = nullptr;
  }
  g.lda = g.K;
  g.theta = theta;
  g.theta_pstride = theta_ps;
  g.w_off = m->w_off[l];
  g.out = m->act[l];
  g.out_pstride = (long long)m->max_batch * g.N;
  g.act = m->acts[l];
  g.vec = (g.K % 8 == 0) && aligned16(g.in) ? 1 : 0;
  g.ctl = ctl;
  if (l == 0 && m->pend_on && ctl == m->ctl) {  // first kernel of an eager step: carries the step scalars
    g.init = m->pend;
    g.init_on = 1;
    m->pend_on = false;
  }
  return g;
}

// forward over layers [0, l_end); activations land in m->act[l]
void launch_forward(pyz_mlp *m, const float *theta, long long theta_ps, int P, const float *x,
                    const int32_t *row_idx, int grid_batch, const StepCtl *ctl, hipStream_t st,
                    float *gather_out = nullptr, int l_end = -1, const StepCtl *gate = nullptr, int gate_mod = 0,
                    long long x_pstride = 0, int l_begin = 0) {
  if (l_end < 0) l_end = m->L;
  for (int l = l_begin; l < l_end; ++l) {
    DenseArgs g = forward_args(m, l, theta, theta_ps, x, row_idx, ctl, gather_out);
    if (l == 0) g.in_pstride = x_pstride;   // (a conv net's Dense tail: one set of rows, the stem's features, per particle)
    g.wt = pyz_wt_for(P);
    g.gate = gate;
    g.gate_mod = gate_mod;
    if (pyz_launch_fwd_ring(g, grid_batch, P, st)) continue;   // mid-size launches: 32-row blocks through the LDS-DMA ring
    if (!g.row_idx && !g.init_on && !g.gather_out) g.rows_cap = std::min(grid_batch, m->max_batch);   // (layer 0 of a caller-owned x: its rows cover grid_batch by contract)
    pyz_launch_fwd(g, grid_batch, P, st);
  }
}

void launch_loss(pyz_mlp *m, int P, const void *y, const int32_t *row_idx, int grid_batch, const StepCtl *ctl,
                 bool want_delta, hipStream_t st) {
  LossArgs g{};
  const int C = m->dims[m->L];
  g.out_last = m->act[m->L - 1];
  g.pstride = (long long)m->max_batch * C;
  g.C = C;
  g.y = y;
  g.delta = want_delta ? m->delta[m->L - 1] : nullptr;
  g.part = m->part;
  g.nblk = cdiv(m->max_batch, 256);
  g.act_last = m->acts[m->L - 1];
  g.ctl = ctl;
  g.row_idx = row_idx;
  dim3 grid(cdiv(grid_batch, 256), P);
  // partial slots of blocks past grid_batch must read as zero: the finalisers sum nblk of them
  if ((int)grid.x < g.nblk) g.nblk = grid.x;
  if (m->loss == PYZ_LOSS_SCCE)
    PYZ_LAUNCH(k_loss_scce, grid, dim3(256), 0, st, g);
  else
    PYZ_LAUNCH(k_loss_mse, grid, dim3(256), 0, st, g);
}

inline int loss_nblk(const pyz_mlp *m, int grid_batch) { return std::min(cdiv(m->max_batch, 256), cdiv(grid_batch, 256)); }

// The Dense tail of a conv net (pyz_convnet_*): its rows x are the stem's features, one set per particle; its gradient block
// sits inside the (P, D_total) gradient of the whole vector; and layer 0 has a data gradient too, towards the features.
struct TailOf {
  long long x_pstride;      // particle stride of x (and of dfeat)
  long long grad_pstride;   // row stride of grad
  float *dfeat;             // (P, max_batch, dims[0]): d loss / d features, times act_feat' of the features
  int act_feat;
};

// grad_sq (one chain only): the weight-gradient kernels also write the batch mean of the squared per-example gradients there
void launch_backward(pyz_mlp *m, const float *theta, long long theta_ps, int P, const float *x,
                     const int32_t *row_idx, int grid_batch, const StepCtl *ctl, float *grad, hipStream_t st,
                     float *grad_sq = nullptr, const TailOf *tail = nullptr) {
  for (int l = m->L - 1; l >= 0; --l) {
    const int K = m->dims[l], N = m->dims[l + 1];
    if (l > 0 || tail) {  // delta[l-1] = (delta[l] W_l^T) * act'(h_{l-1}); layer 0 of a tail: the same towards the features
      DenseArgs g{};
      g.K = K;
      g.N = N;
      g.in = m->delta[l];
      g.in_pstride = (long long)m->max_batch * N;
      g.lda = N;
      g.theta = theta;
      g.theta_pstride = theta_ps;
      g.w_off = m->w_off[l];
      g.out = l > 0 ? m->delta[l - 1] : tail->dfeat;
      g.out_pstride = l > 0 ? (long long)m->max_batch * K : tail->x_pstride;
      g.aux = l > 0 ? m->act[l - 1] : x;
      g.aux_pstride = g.out_pstride;
      g.act = l > 0 ? m->acts[l - 1] : tail->act_feat;
      g.vec = (N % 8 == 0) && (m->w_off[l] % 4 == 0) && (P == 1 || theta_ps % 4 == 0) && aligned16(theta) ? 1 : 0;
      g.ctl = ctl;
      pyz_launch_bwd_data(g, grid_batch, P, st);
    }
    DenseArgs g{};
    g.K = K;
    g.N = N;
    if (l == 0) {
      g.in = x;
      g.in_pstride = tail ? tail->x_pstride : 0;
      g.row_idx = row_idx;
    } else {
      g.in = m->act[l - 1];
      g.in_pstride = (long long)m->max_batch * K;
    }
    g.lda = K;
    g.aux = m->delta[l];
    g.aux_pstride = (long long)m->max_batch * N;
    g.out = grad;
    g.out_pstride = tail ? tail->grad_pstride : m->D;
    g.w_off = m->w_off[l];
    g.ctl = ctl;
    if (grad_sq) pyz_launch_bwd_weight_sq(g, grad_sq, grid_batch, st);
    else pyz_launch_bwd_weight(g, grid_batch, P, st);
  }
}

// ---- fused path (pyz_fused.h): usable when the last layer fits one 32-wide tile
inline bool can_fuse(const pyz_mlp *m) { return m->dims[m->L] <= 32; }

void launch_head(pyz_mlp *m, const float *theta, long long theta_ps, int P, const float *x, const void *y,
                 const int32_t *row_idx, int grid_batch, const StepCtl *ctl, bool want_delta, hipStream_t st,
                 const StepCtl *gate = nullptr, int gate_mod = 0, int k_split = 0) {
  const int l = m->L - 1;
  HeadArgs g{};
  g.gate = gate;
  g.gate_mod = gate_mod;
  if (k_split > 1) {   // the hidden layer arrives as the partial sums of a split-reduction forward (ksplit_forward_ok)
    g.hparts = static_cast<const float *>(full(m)->x.fwd_part);
    g.n_hparts = k_split;
    g.hpart_stride = (long long)m->max_batch * m->dims[l];
    g.bias_prev = theta + m->w_off[l - 1] + (long long)m->dims[l - 1] * m->dims[l];
    g.h_store = m->act[l - 1];
  }
  g.K = m->dims[l];
  g.N = m->dims[l + 1];
  if (l == 0) {
    g.hin = x;
    g.hin_pstride = 0;
    g.gather_hin = 1;
  } else {
    g.hin = m->act[l - 1];
    g.hin_pstride = (long long)m->max_batch * g.K;
    g.gather_hin = 0;
  }
  g.lda = g.K;
  g.row_idx = row_idx;
  g.theta = theta;
  g.theta_pstride = theta_ps;
  g.w_off = m->w_off[l];
  g.loss = m->loss;
  g.act_last = m->acts[l];
  g.act_prev = l > 0 ? m->acts[l - 1] : PYZ_ACT_LINEAR;
  g.vec = (g.K % 8 == 0) && aligned16(g.hin) ? 1 : 0;
  g.y = y;
  g.out_last = m->act[l];
  g.delta_last = want_delta ? m->delta[l] : nullptr;
  g.delta_prev = (want_delta && l > 0) ? m->delta[l - 1] : nullptr;
  g.last_pstride = (long long)m->max_batch * g.N;
  g.prev_pstride = (long long)m->max_batch * g.K;
  g.part = m->part;
  g.ctl = ctl;
  g.wt = pyz_wt_for(P);
  if (m->pend_on && ctl == m->ctl) {  // no hidden layer: the head is the first kernel of the eager step
    g.init = m->pend;
    g.init_on = 1;
    m->pend_on = false;
  }
  // one wave per batch row when the lane-resident operands fit (UT units x NP classes per lane)
  static const int rows_on = pyz_env_int("PYZ_HEAD_ROWS", 1);
  const int UT = g.K <= 64 ? 1 : g.K <= 256 ? 4 : g.K <= 512 ? 8 : g.K <= 1024 ? 16 : 0;
  const int NP = g.N <= 4 ? 4 : g.N <= 8 ? 8 : g.N <= 12 ? 12 : g.N <= 16 ? 16 : g.N <= 24 ? 24 : 32;
  if (rows_on && UT && UT * NP <= 128) {
    g.nblk = grid_batch;  // one loss partial per row
    m->cur_nblk = g.nblk;
    // rows per wave: four when the launch has tens of thousands of rows (many particles), else one
    static const int rw_rows = pyz_env_int("PYZ_HEAD_RW_ROWS", 32768);
    const int RW = (long long)P * grid_batch >= rw_rows ? 4 : 1;
    const dim3 grid((unsigned)cdiv(cdiv(grid_batch, RW), 4), P), block(256);
    if (g.n_hparts > 0) {   // behind a split-reduction forward (ksplit_for: UT == 4, at most 16 classes, one chain)
      if (NP == 4) PYZ_LAUNCH((k_head_rows<4, 4, 1, true>), grid, block, 0, st, g);
      else if (NP == 8) PYZ_LAUNCH((k_head_rows<4, 8, 1, true>), grid, block, 0, st, g);
      else if (NP == 12) PYZ_LAUNCH((k_head_rows<4, 12, 1, true>), grid, block, 0, st, g);
      else PYZ_LAUNCH((k_head_rows<4, 16, 1, true>), grid, block, 0, st, g);
      return;
    }
#define PYZ_HEAD_ROWS_CASE(U, C)                                                               \
  if (UT == U && NP == C) {                                                                    \
    if (RW == 4) PYZ_LAUNCH((k_head_rows<U, C, 4>), grid, block, 0, st, g);                     \
    else PYZ_LAUNCH((k_head_rows<U, C, 1>), grid, block, 0, st, g);                            \
    return;                                                                                    \
  }
    PYZ_HEAD_ROWS_CASE(1, 4) PYZ_HEAD_ROWS_CASE(1, 8) PYZ_HEAD_ROWS_CASE(1, 12) PYZ_HEAD_ROWS_CASE(1, 16)
    PYZ_HEAD_ROWS_CASE(1, 24) PYZ_HEAD_ROWS_CASE(1, 32)
    PYZ_HEAD_ROWS_CASE(4, 4) PYZ_HEAD_ROWS_CASE(4, 8) PYZ_HEAD_ROWS_CASE(4, 12) PYZ_HEAD_ROWS_CASE(4, 16)
    PYZ_HEAD_ROWS_CASE(4, 24) PYZ_HEAD_ROWS_CASE(4, 32)
    PYZ_HEAD_ROWS_CASE(8, 4) PYZ_HEAD_ROWS_CASE(8, 8) PYZ_HEAD_ROWS_CASE(8, 12) PYZ_HEAD_ROWS_CASE(8, 16)
    PYZ_HEAD_ROWS_CASE(16, 4) PYZ_HEAD_ROWS_CASE(16, 8)
#undef PYZ_HEAD_ROWS_CASE
  }
  g.nblk = cdiv(grid_batch, 32);
  m->cur_nblk = g.nblk;
  static const int head_waves = pyz_env_int("PYZ_HEAD_WAVES", 8) >= 8 ? 8 : 4;
  PYZ_LAUNCH(k_head, dim3(g.nblk, P), dim3(64 * head_waves), head_waves * 4096 + 2 * 32 * 33 * 4 + 64, st, g);
}

// data gradients of layers L-2 .. 1 (the head already produced delta[L-2])
void launch_bwd_data_hidden(pyz_mlp *m, const float *theta, long long theta_ps, int P, int grid_batch,
                            const StepCtl *ctl, hipStream_t st) {
  for (int l = m->L - 2; l >= 1; --l) {
    const int K = m->dims[l], N = m->dims[l + 1];
    DenseArgs g{};
    g.K = K;
    g.N = N;
    g.in = m->delta[l];
    g.in_pstride = (long long)m->max_batch * N;
    g.lda = N;
    g.theta = theta;
    g.theta_pstride = theta_ps;
    g.w_off = m->w_off[l];
    g.out = m->delta[l - 1];
    g.out_pstride = (long long)m->max_batch * K;
    g.aux = m->act[l - 1];
    g.aux_pstride = (long long)m->max_batch * K;
    g.act = m->acts[l - 1];
    g.vec = (N % 8 == 0) && (m->w_off[l] % 4 == 0) && (P == 1 || theta_ps % 4 == 0) && aligned16(theta) ? 1 : 0;
    g.ctl = ctl;
    pyz_launch_bwd_data(g, grid_batch, P, st);
  }
}

inline int wgrad_tiles(const pyz_mlp *m) {   // workgroups of k_wgrad_all that own a 32 x 32 tile (launch_wgrad_all's count)
  int tiles = 0;
  for (int l = 0; l < m->L; ++l) tiles += ((m->dims[l] + 1 + 31) / 32) * ((m->dims[l + 1] + 31) / 32);
  return tiles;
}

// the layers, tiles and duties of a weight-gradient launch (k_wgrad_all, k_wgrad_adam); returns the tile count
int wgrad_layers(pyz_mlp *m, int P, const float *x, const int32_t *row_idx, const StepCtl *ctl, WgradArgs &a,
                 const float *gathered) {
  int tiles = 0;
  a.L = m->L;
  for (int l = 0; l < m->L; ++l) {
    WgradLayer &ly = a.lay[l];
    ly.K = m->dims[l];
    ly.N = m->dims[l + 1];
    if (l == 0) {
      ly.in = (row_idx && gathered) ? gathered : x;  // the forward pass left a contiguous copy of the batch rows
      ly.in_pstride = 0;
      ly.gather = (row_idx && !gathered) ? 1 : 0;
    } else {
      ly.in = m->act[l - 1];
      ly.in_pstride = (long long)m->max_batch * ly.K;
      ly.gather = 0;
    }
    ly.lda = ly.K;
    ly.delta = m->delta[l];
    ly.delta_pstride = (long long)m->max_batch * ly.N;
    ly.w_off = m->w_off[l];
    ly.tile0 = tiles;
    a.tile0[l] = tiles;
    tiles += ((ly.K + 1 + 31) / 32) * ((ly.N + 31) / 32);
  }
  for (int l = m->L; l < PYZ_MAX_LAYERS; ++l) a.tile0[l] = INT_MAX;   // no tile id reaches it
  a.row_idx = row_idx;
  a.ctl = ctl;
  a.part = m->part;
  a.nblk = m->cur_nblk;
  a.tiles = tiles;
  a.nonfinite = m->nonfinite;
  a.wt = pyz_wt_for(P);
  return tiles;
}

// every layer's weight gradient in one launch; `a` carries the update mode and its buffers
void launch_wgrad_all(pyz_mlp *m, int P, const float *x, const int32_t *row_idx, int grid_batch, const StepCtl *ctl,
                      WgradArgs &a, hipStream_t st, const float *gathered) {
  const int tiles = wgrad_layers(m, P, x, row_idx, ctl, a, gathered);
  const int S = pyz_pick_waves((long long)tiles * P, (grid_batch + 1) / 2);
  dim3 grid(pyz_pad8((long long)tiles + 1, P), P);  // + the duties workgroup (+ padding, see pyz_pad8)
  if (a.prep.src && P == 1) grid.x = (unsigned)(tiles + 1 + std::max(pyz_cu_count() - tiles - 1, 24));  // + the batch workers
  switch (S) {
    case 1:
      if (a.mode == PYZ_UPD_NONE) PYZ_LAUNCH((k_wgrad_all<1, true>), grid, dim3(64), 0, st, a);
      else PYZ_LAUNCH(k_wgrad_all<1>, grid, dim3(64), 0, st, a);
      break;
    case 2: PYZ_LAUNCH(k_wgrad_all<2>, grid, dim3(128), 2 * 4096, st, a); break;
    case 4: PYZ_LAUNCH(k_wgrad_all<4>, grid, dim3(256), 4 * 4096, st, a); break;
    case 8: PYZ_LAUNCH(k_wgrad_all<8>, grid, dim3(512), 8 * 4096, st, a); break;
    default: PYZ_LAUNCH(k_wgrad_all<16>, grid, dim3(1024), 16 * 4096, st, a); break;
  }
}

// launch_wgrad_all of a run that keeps its batches as images (one chain, an updating mode): layer 0 reads this step's
// weight-gradient image wimg, and the workers leave the next batch as images too (a.prep.dst is a slot of images).  The same
// tiles, waves and grid.
void launch_wgrad_all_frag(pyz_mlp *m, const float *x, const int32_t *row_idx, int grid_batch, const StepCtl *ctl, WgradArgs &a,
                           hipStream_t st, const float *wimg) {
  const int tiles = wgrad_layers(m, 1, x, row_idx, ctl, a, wimg);
  const int S = pyz_pick_waves(tiles, (grid_batch + 1) / 2);
  dim3 grid((unsigned)tiles + 1);  // + the duties workgroup
  if (a.prep.src) grid.x = (unsigned)(tiles + 1 + std::max(pyz_cu_count() - tiles - 1, 24));  // + the batch workers
  a.lay[0].lda = 8 * ((m->max_batch + 7) / 8);   // rows of the image
  switch (S) {
    case 1: PYZ_LAUNCH_AS(k_wgrad_all<1>, k_wgrad_all_frag<1>, grid, dim3(64), 0, st, a); break;
    case 2: PYZ_LAUNCH_AS(k_wgrad_all<2>, k_wgrad_all_frag<2>, grid, dim3(128), 2 * 4096, st, a); break;
    case 4: PYZ_LAUNCH_AS(k_wgrad_all<4>, k_wgrad_all_frag<4>, grid, dim3(256), 4 * 4096, st, a); break;
    case 8: PYZ_LAUNCH_AS(k_wgrad_all<8>, k_wgrad_all_frag<8>, grid, dim3(512), 8 * 4096, st, a); break;
    default: PYZ_LAUNCH_AS(k_wgrad_all<16>, k_wgrad_all_frag<16>, grid, dim3(1024), 16 * 4096, st, a); break;
  }
}

// ADAM / VADAM (one chain): every layer's gradient and squared-gradient mean, and the update, in one launch
void launch_wgrad_adam(pyz_mlp *m, const float *x, const int32_t *row_idx, int grid_batch, const StepCtl *ctl, AdamArgs &a,
                       hipStream_t st, const float *gathered) {
  const int tiles = wgrad_layers(m, 1, x, row_idx, ctl, a.w, gathered);
  const int S = pyz_pick_waves(tiles, (grid_batch + 1) / 2);
  const dim3 grid(tiles + 1);   // + the duties workgroup
  switch (S) {
    case 1: PYZ_LAUNCH(k_wgrad_adam<1>, grid, dim3(64), 0, st, a); break;
    case 2: PYZ_LAUNCH(k_wgrad_adam<2>, grid, dim3(128), 2 * 4096, st, a); break;
    case 4: PYZ_LAUNCH(k_wgrad_adam<4>, grid, dim3(256), 4 * 4096, st, a); break;
    case 8: PYZ_LAUNCH(k_wgrad_adam<8>, grid, dim3(512), 8 * 4096, st, a); break;
    default: PYZ_LAUNCH(k_wgrad_adam<16>, grid, dim3(1024), 16 * 4096, st, a); break;
  }
}

// BSAM (one chain): every layer's gradient and the ascent (phase 0) or the update (phase 1) in one launch
void launch_wgrad_bsam(pyz_mlp *m, const float *x, const int32_t *row_idx, int grid_batch, const StepCtl *ctl, int phase,
                       BsamArgs &a, hipStream_t st, const float *gathered) {
  const int tiles = wgrad_layers(m, 1, x, row_idx, ctl, a.w, gathered);
  const int S = pyz_pick_waves(tiles, (grid_batch + 1) / 2);
  const dim3 grid(tiles + 1);   // + the duties workgroup
#define PYZ_BSAM_CASE(W, LDS)                                                           \
  if (phase == 0) PYZ_LAUNCH((k_wgrad_bsam<W, 0>), grid, dim3(64 * W), LDS, st, a);     \
  else PYZ_LAUNCH((k_wgrad_bsam<W, 1>), grid, dim3(64 * W), LDS, st, a);                \
  break
  switch (S) {
    case 1: PYZ_BSAM_CASE(1, 0);
    case 2: PYZ_BSAM_CASE(2, 2 * 4096);
    case 4: PYZ_BSAM_CASE(4, 4 * 4096);
    case 8: PYZ_BSAM_CASE(8, 8 * 4096);
    default: PYZ_BSAM_CASE(16, 16 * 4096);
  }
#undef PYZ_BSAM_CASE
}

inline float *batch_buf(pyz_mlp *m, int slot) { return m->xb + (size_t)slot * m->max_batch * m->dims[0]; }

// chained runs whose batches are assembled one step ahead (PrepArgs, pyz_fused.h): single chain, fused path, a hidden layer
// ... and a weight-gradient launch that leaves CUs idle for the copy: with more tiles than CUs (C4: 507) the workers only
// take CUs from the tiles (72.6 against 71.7 us per step at C4; C2, 182 tiles: 24.4 against 26.7 the other way).
// PYZ_BATCH_AHEAD=2 forces it on for every shape.
inline bool batch_ahead(const pyz_mlp *m, const int32_t *row_idx) {
  static const int on = pyz_env_int("PYZ_BATCH_AHEAD", 1);
  if (!on || !can_fuse(m) || m->L <= 1 || row_idx == nullptr) return false;
  return on == 2 || wgrad_tiles(m) + 24 <= pyz_cu_count();
}

// The image form of the batches assembled ahead (PrepArgs, pyz_fused.h): a slot is the forward image and the weight-gradient
// image behind it.  PYZ_BATCH_FRAG [1] is read when the plan is created (the images are larger than the two row-major copies).
inline size_t frag_fwd_floats(const pyz_mlp *m) { return (size_t)((m->max_batch + 31) / 32) * 32 * m->dims[0]; }
inline size_t frag_slot_floats(const pyz_mlp *m) {
  return frag_fwd_floats(m) + (size_t)((m->dims[0] + 31) / 32) * ((m->max_batch + 7) / 8) * 256;
}
inline float *frag_buf(pyz_mlp *m, int slot) { return m->xb + (size_t)slot * frag_slot_floats(m); }

// Does this run keep its batches as images?  Only where layer 0's forward is k_dense_fwd and the weight gradients are
// k_wgrad_all with `theta` the weights it multiplies: the SGD / SGLD / SWAG / BBB runs of sgld_run_impl, one chain.
bool batch_frag(pyz_mlp *m, const float *theta, const float *x, const int32_t *row_idx, int grid_batch) {
  if (!m->frag_on || !batch_ahead(m, row_idx)) return false;
  const int K = m->dims[0];
  if (K % 8 || !aligned16(x) || !aligned16(m->xb)) return false;
  if (pyz_env_int("PYZ_FWD_KSPLIT", 0) >= 2) return false;   // (the split-reduction forward reads rows)
  DenseArgs g = forward_args(m, 0, theta, m->D, frag_buf(m, 0), nullptr, nullptr, nullptr);
  if (!g.vec || pyz_fwd_ring_variant(g, grid_batch, 1)) return false;
  const long long tiles = (long long)((grid_batch + 31) / 32) * ((g.N + 31) / 32);
  return !pyz_fwd_takes_lds(g, grid_batch, 1, pyz_pick_waves(tiles, (g.K + 1) / 2 + 1));
}

PrepArgs prep_args(pyz_mlp *m, const float *x, const int32_t *row_idx, int grid_batch, long long row_stride, int dst_slot) {
  PrepArgs p{};
  p.src = x;
  p.dst = batch_buf(m, dst_slot);
  p.row_idx = row_idx;
  p.tab_bs = m->tab_bs;
  p.row_stride = row_stride;
  p.K = p.lda = m->dims[0];
  p.fwd_tiles_n = (m->dims[1] + 31) / 32;
  p.fwd_tiles = ((grid_batch + 31) / 32) * p.fwd_tiles_n;
  return p;
}

// prep_args of a run that keeps its batches as images: the destination is a slot of images
inline PrepArgs frag_prep(pyz_mlp *m, PrepArgs p, int dst_slot) {
  p.dst = frag_buf(m, dst_slot);
  return p;
}

// forward + loss (+ backward into `grad` when upd.mode == NONE and grad given, or the fused update).
// ahead_slot >= 0 (chained runs): this step's rows already stand in batch_buf(ahead_slot), and upd.prep says where the
// weight-gradient launch assembles the next step's.
// split-reduction forward (k_dense_fwd_ring, k_split) + partial-summing head for this launch?  Returns the split (0: no).
int ksplit_for(pyz_mlp *m, const float *theta, long long theta_ps, int P, const float *xc, int grid_batch, const StepCtl *ctl) {
  // Opt-in (read when a run's graph is captured): measured SLOWER at C2 -- 27.5 us per step with 8 ranges, 30.3 with 4, against
  // 24.6 (the forward ~10.7 us against 8.5: seven slabs do not amortise the ring's prologue and the 6.5 MB of partial sums;
  // the head 6.6 against 4.6 us: 32 loads per lane instead of 4) -- profiles/r03_ksplit/.
  const int ks_env = pyz_env_int("PYZ_FWD_KSPLIT", 0);
  if (ks_env < 2 || ks_env > 8 || m->L != 2 || P != 1) return 0;
  const int UT = m->dims[1] <= 64 ? 1 : m->dims[1] <= 256 ? 4 : 0, NPc = m->dims[2];
  if (!UT || NPc > 16 || !pyz_env_int("PYZ_HEAD_ROWS", 1)) return 0;          // the head must be k_head_rows
  DenseArgs g = forward_args(m, 0, theta, theta_ps, xc, nullptr, ctl, nullptr);
  if (!pyz_fwd_ring_ksplit_ok(g, grid_batch, P)) return 0;
  if ((long long)((grid_batch + 31) / 32) * ks_env > 2 * pyz_cu_count()) return 0;   // (already enough row blocks)
  // (the buffer of partial sums is allocated with the plan: this runs inside stream capture, where nothing may be allocated)
  const size_t need = sizeof(float) * (size_t)ks_env * m->max_batch * m->dims[1];
  if (!full(m)->x.fwd_part || full(m)->x.fwd_part_cap < need) return 0;
  return ks_env;
}

// adam (one chain, no ahead_slot): the weight-gradient launch is k_wgrad_adam with a.w = upd (fused path), or the
// squared-gradient kernels write their means to grad2 beside upd.grad (unfused path)
void launch_loss_backward(pyz_mlp *m, const float *theta, long long theta_ps, int P, const float *x, const void *y,
                          const int32_t *row_idx, int grid_batch, const StepCtl *ctl, bool want_grad, WgradArgs &upd,
                          hipStream_t st, int ahead_slot = -1, AdamArgs *adam = nullptr, bool frag = false) {
  if (can_fuse(m)) {
    if (ahead_slot >= 0 && frag) {   // this step's rows stand as images in frag_buf(ahead_slot) (batch_frag)
      DenseArgs g = forward_args(m, 0, theta, theta_ps, frag_buf(m, ahead_slot), nullptr, ctl, nullptr);
      g.wt = pyz_wt_for(P);
      g.rows_cap = std::min(grid_batch, m->max_batch);
      pyz_launch_fwd_frag(g, grid_batch, st);
      launch_forward(m, theta, theta_ps, P, nullptr, nullptr, grid_batch, ctl, st, nullptr, m->L - 1, nullptr, 0, 0, 1);
      launch_head(m, theta, theta_ps, P, x, y, row_idx, grid_batch, ctl, want_grad, st);   // (labels go through row_idx)
      launch_bwd_data_hidden(m, theta, theta_ps, P, grid_batch, ctl, st);
      launch_wgrad_all_frag(m, x, row_idx, grid_batch, ctl, upd, st, frag_buf(m, ahead_slot) + frag_fwd_floats(m));
      return;
    }
    if (ahead_slot >= 0) {
      const float *xc = batch_buf(m, ahead_slot);
      // one hidden layer of <= 200 units, one chain: the forward with its reduction split over PYZ_FWD_KSPLIT workgroups per
      // row block, the head adds the partial sums (see pyz_gemm_ring.h)
      const int ks = ksplit_for(m, theta, theta_ps, P, xc, grid_batch, ctl);
      if (ks > 1) {
        DenseArgs g = forward_args(m, 0, theta, theta_ps, xc, nullptr, ctl, nullptr);
        g.wt = pyz_wt_for(P);
        g.k_split = ks;
        g.part_out = static_cast<float *>(full(m)->x.fwd_part);
        g.part_stride = (long long)m->max_batch * g.N;
        pyz_launch_fwd_ring_ksplit(g, grid_batch, st);
      } else {
        launch_forward(m, theta, theta_ps, P, xc, nullptr, grid_batch, ctl, st, nullptr, m->L - 1);
      }
      launch_head(m, theta, theta_ps, P, x, y, row_idx, grid_batch, ctl, want_grad, st, nullptr, 0, ks);   // (labels go through row_idx)
      launch_bwd_data_hidden(m, theta, theta_ps, P, grid_batch, ctl, st);
      launch_wgrad_all(m, P, x, row_idx, grid_batch, ctl, upd, st, xc);
      return;
    }
    static const int use_xb = pyz_env_int("PYZ_GATHER_COPY", 1);  // 1: forward leaves a contiguous batch copy
    float *xb = (use_xb && want_grad && row_idx && m->L > 1) ? m->xb : nullptr;
    launch_forward(m, theta, theta_ps, P, x, row_idx, grid_batch, ctl, st, xb, m->L - 1);   // hidden layers
    launch_head(m, theta, theta_ps, P, x, y, row_idx, grid_batch, ctl, want_grad, st);
    if (want_grad) {
      launch_bwd_data_hidden(m, theta, theta_ps, P, grid_batch, ctl, st);
      if (adam) launch_wgrad_adam(m, x, row_idx, grid_batch, ctl, *adam, st, xb);
      else launch_wgrad_all(m, P, x, row_idx, grid_batch, ctl, upd, st, xb);
    }
    return;
  }
  flush_ctl(m, st);
  launch_forward(m, theta, theta_ps, P, x, row_idx, grid_batch, ctl, st);
  launch_loss(m, P, y, row_idx, grid_batch, ctl, want_grad, st);
  m->cur_nblk = loss_nblk(m, grid_batch);
  if (want_grad) launch_backward(m, theta, theta_ps, P, x, row_idx, grid_batch, ctl, upd.grad, st, adam ? m->grad2 : nullptr);
}

// one gradient pass of a BSAM step on the fused path (launch_loss_backward's eager sequence): forward, head, data
// gradients of the hidden layers, then k_wgrad_bsam<phase> with its epilogue
void launch_bsam_pass(pyz_mlp *m, const float *theta, const float *x, const void *y, const int32_t *row_idx, int grid_batch,
                      int phase, BsamArgs &a, hipStream_t st) {
  static const int use_xb = pyz_env_int("PYZ_GATHER_COPY", 1);  // 1: forward leaves a contiguous batch copy
  float *xb = (use_xb && row_idx && m->L > 1) ? m->xb : nullptr;
  launch_forward(m, theta, m->D, 1, x, row_idx, grid_batch, m->ctl, st, xb, m->L - 1);   // hidden layers
  launch_head(m, theta, m->D, 1, x, y, row_idx, grid_batch, m->ctl, true, st);
  launch_bwd_data_hidden(m, theta, m->D, 1, grid_batch, m->ctl, st);
  launch_wgrad_bsam(m, x, row_idx, grid_batch, m->ctl, phase, a, st, xb);
}

int check_loss_combo(const pyz_mlp *m) {
  const int last = m->acts[m->L - 1];
  if (m->loss == PYZ_LOSS_SCCE && last != PYZ_ACT_SOFTMAX)
    return pyz_fail(PYZ_E_INVALID, "SparseCategoricalCrossentropy needs a softmax last layer");
  if (m->loss == PYZ_LOSS_MSE && last == PYZ_ACT_SOFTMAX)
    return pyz_fail(PYZ_E_INVALID, "MeanSquaredError on a softmax last layer is not supported");
  if (m->loss == PYZ_LOSS_BCE && (m->dims[m->L] != 1 || last != PYZ_ACT_SIGMOID))
    return pyz_fail(PYZ_E_INVALID, "BinaryCrossentropy needs a last layer of exactly one sigmoid unit");
  return PYZ_OK;
}

// the update's scalars, each computed in float64 and rounded to float32 once (see AdamScal)
AdamScal adam_scalars(float lr, double beta_1, double beta_2, long long epoch, float denom_eps, float decay) {
  AdamScal a;
  a.lr = lr;
  a.b1 = (float)beta_1;
  a.c1 = (float)(1.0 - beta_1);
  a.b2 = (float)beta_2;
  a.c2 = (float)(1.0 - beta_2);
  a.bc1 = (float)(1.0 - std::pow(beta_1, (double)epoch));
  a.bc2 = (float)(1.0 - std::pow(beta_2, (double)epoch));
  a.eps = denom_eps;
  a.decay = decay;
  return a;
}

// delta[0] of every draw of a chunk (pyz_input_grad): forward, head / loss, and the data gradients down to layer 1 -- the
// sequences of launch_loss_backward without their weight-gradient launches
void launch_delta0(pyz_mlp *m, const float *theta, int P, const float *x, const void *y, int n, hipStream_t st) {
  if (can_fuse(m)) {
    launch_forward(m, theta, m->D, P, x, nullptr, n, m->ctl, st, nullptr, m->L - 1);   // hidden layers
    launch_head(m, theta, m->D, P, x, y, nullptr, n, m->ctl, true, st);                // leaves delta[L-1] and delta[L-2]
    launch_bwd_data_hidden(m, theta, m->D, P, n, m->ctl, st);
    return;
  }
  launch_forward(m, theta, m->D, P, x, nullptr, n, m->ctl, st);
  launch_loss(m, P, y, nullptr, n, m->ctl, true, st);
  m->cur_nblk = loss_nblk(m, n);
  if (m->L > 1) {   // delta[L-2] = (delta[L-1] W_{L-1}^T) * act'(h_{L-2}): the layer launch_bwd_data_hidden leaves to the head
    const int l = m->L - 1, K = m->dims[l], N = m->dims[l + 1];
    DenseArgs g{};
    g.K = K;
    g.N = N;
    g.in = m->delta[l];
    g.in_pstride = (long long)m->max_batch * N;
    g.lda = N;
    g.theta = theta;
    g.theta_pstride = m->D;
    g.w_off = m->w_off[l];
    g.out = m->delta[l - 1];
    g.out_pstride = (long long)m->max_batch * K;
    g.aux = m->act[l - 1];
    g.aux_pstride = (long long)m->max_batch * K;
    g.act = m->acts[l - 1];
    g.vec = (N % 8 == 0) && (m->w_off[l] % 4 == 0) && (P == 1 || m->D % 4 == 0) && aligned16(theta) ? 1 : 0;
    g.ctl = m->ctl;
    pyz_launch_bwd_data(g, n, P, st);
  }
  launch_bwd_data_hidden(m, theta, m->D, P, n, m->ctl, st);
}

// ---------------------------------------------------------------- conv nets: the stem's host side
// rows of one range of the weight-gradient reduction: a function of the plan alone, so the split (and with it the order
// of the sums) does not depend on the batch of the call
inline int stem_rows_per_range(const pyz_stem *s, const StemOp &o) {
  const long long m_max = (long long)s->max_batch * o.OH * o.OW;
  return (int)std::max<long long>(256, ((m_max + 255) / 256 + 1) / 2 * 2);
}

int stem_check(const pyz_stem *s, int P, int batch) {
  if (!s) return pyz_fail(PYZ_E_INVALID, "null stem");
  if (batch <= 0 || batch > s->max_batch) return pyz_fail(PYZ_E_SHAPE, "batch %d outside [1, %d] of the plan", batch, s->max_batch);
  if (P <= 0 || P > s->max_p) return pyz_fail(PYZ_E_SHAPE, "particle count %d outside [1, %d] of the plan", P, s->max_p);
  return PYZ_OK;
}

ConvArgs conv_args(const pyz_stem *s, int o, const float *theta, long long theta_ps, const float *x, const int32_t *row_idx, int batch) {
  const StemOp &c = s->op[o];
  ConvArgs g{};
  if (o == 0) {
    g.in = x;
    g.in_pstride = 0;
    g.row_idx = row_idx;
  } else {
    g.in = s->op[o - 1].out;
    g.in_pstride = (long long)s->max_batch * s->op[o - 1].size();
  }
  g.theta = theta;
  g.theta_pstride = theta_ps;
  g.w_off = c.w_off;
  g.out = c.out;
  g.out_pstride = (long long)s->max_batch * c.size();
  g.delta = c.delta;
  g.delta_pstride = g.out_pstride;
  g.ktab = c.ktab;
  g.batch = batch;
  g.M = batch * c.OH * c.OW;
  g.H = c.H; g.W = c.W; g.C = c.C; g.OH = c.OH; g.OW = c.OW; g.N = c.N; g.K = c.K; g.KT = c.KT;
  g.kh = c.kh; g.kw = c.kw; g.pt = c.pt; g.pl = c.pl; g.act = c.act;
  g.inv_ohw = 1.0f / (float)(c.OH * c.OW);
  g.inv_ow = 1.0f / (float)c.OW;
  return g;
}

PoolArgs pool_args(const pyz_stem *s, int o, int batch) {
  const StemOp &q = s->op[o], &c = s->op[o - 1];
  PoolArgs g{};
  g.in = c.out;
  g.in_pstride = (long long)s->max_batch * c.size();
  g.out = q.out;
  g.out_pstride = (long long)s->max_batch * q.size();
  g.win = q.win;
  g.dout = q.delta;
  g.din = c.delta;
  g.batch = batch;
  g.H = q.H; g.W = q.W; g.C = q.C; g.OH = q.OH; g.OW = q.OW; g.ph = q.kh; g.pw = q.kw;
  g.act_below = c.act;
  return g;
}

inline int conv_waves(long long tiles, int steps) {
  int S = 1;
  while (S < PYZ_CONV_WAVES && tiles * S < 1024 && steps >= 16 * S) S *= 2;
  return S;
}

// every op's output into the workspace; the last one's is the features (P, max_batch, F)
void stem_forward(pyz_stem *s, const float *theta, long long theta_ps, int P, const float *x, const int32_t *row_idx, int batch,
                  hipStream_t st) {
  for (int o = 0; o < s->n_ops; ++o) {
    const StemOp &c = s->op[o];
    if (c.kind == PYZ_STEM_CONV) {
      ConvArgs g = conv_args(s, o, theta, theta_ps, x, row_idx, batch);
      const long long tiles = (long long)((g.M + 31) / 32) * ((g.N + 31) / 32);
      const int S = conv_waves(tiles * P, g.KT / 2);
      PYZ_LAUNCH(k_conv_fwd, dim3((unsigned)tiles, P), dim3(64 * S), (size_t)g.KT * 8 + (S > 1 ? S * 4096 : 0), st, g);
    } else {
      PoolArgs g = pool_args(s, o, batch);
      PYZ_LAUNCH(k_pool_fwd, dim3((unsigned)cdiv((long long)batch * c.size(), 256), P), dim3(256), 0, st, g);
    }
  }
  s->forwarded = true;
}

// bytes of the partial-tile slab of the weight-gradient reductions: the largest conv's (P, G, tiles, 32 x 32)
size_t stem_part_bytes(const pyz_stem *s) {
  size_t need = 0;
  for (int o = 0; o < s->n_ops; ++o) {
    const StemOp &c = s->op[o];
    if (c.kind != PYZ_STEM_CONV) continue;
    const long long tiles = (long long)((c.K + 1 + 31) / 32) * ((c.N + 31) / 32);
    const long long G = cdiv((long long)s->max_batch * c.OH * c.OW, stem_rows_per_range(s, c));
    need = std::max(need, sizeof(float) * (size_t)(s->max_p * G * tiles * 1024));
  }
  return need;
}

// the stem's block of the gradient from the last op's delta (a conv's: d loss / d pre-activation; a pool's: d loss / d out)
void stem_backward(pyz_stem *s, const float *theta, long long theta_ps, int P, const float *x, const int32_t *row_idx, int batch,
                   float *grad, long long grad_ps, hipStream_t st) {
  for (int o = s->n_ops - 1; o >= 0; --o) {
    const StemOp &c = s->op[o];
    if (c.kind == PYZ_STEM_POOL) {
      PoolArgs g = pool_args(s, o, batch);
      PYZ_LAUNCH(k_pool_bwd, dim3((unsigned)cdiv((long long)batch * c.H * c.W * c.C, 256), P), dim3(256), 0, st, g);
      continue;
    }
    ConvArgs g = conv_args(s, o, theta, theta_ps, x, row_idx, batch);
    g.rows_per_g = stem_rows_per_range(s, c);
    g.G = cdiv(g.M, g.rows_per_g);
    g.part = s->part;
    g.grad = grad;
    g.grad_pstride = grad_ps;
    const long long tiles = (long long)((g.K + 1 + 31) / 32) * ((g.N + 31) / 32);
    const int S = conv_waves(tiles * g.G * P, std::min(g.M, g.rows_per_g) / 2);
    PYZ_LAUNCH(k_conv_wgrad, dim3((unsigned)(tiles * g.G), P), dim3(64 * S), (S > 1 ? S * 4096 : 0) + PYZ_WGRAD_CHUNK * 16, st, g);
    PYZ_LAUNCH(k_conv_wgrad_reduce, dim3((unsigned)cdiv((long long)(g.K + 1) * g.N, 16), P), dim3(256), 0, st, g);
    if (o > 0) {   // (not launched for the first conv: nothing is below it)
      const StemOp &b = s->op[o - 1];
      g.out = b.delta;
      g.out_pstride = (long long)s->max_batch * b.size();
      g.below = b.kind == PYZ_STEM_CONV ? b.out : nullptr;
      g.below_pstride = g.out_pstride;
      g.act_below = b.act;
      PYZ_LAUNCH(k_conv_dgrad, dim3((unsigned)cdiv((long long)batch * c.H * c.W * c.C, 256), P), dim3(256), 0, st, g);
    }
  }
}

int convnet_check(const pyz_stem *s, const pyz_mlp *m, int P, int batch) {
  int rc = stem_check(s, P, batch);
  if (rc) return rc;
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  // the conv net's loss goes through launch_loss (k_loss_scce / k_loss_mse), which has no BinaryCrossentropy arm: on a Dense
  // net that loss always takes the fused head (one output unit)
  if (m->loss == PYZ_LOSS_BCE) return pyz_fail(PYZ_E_INVALID, "BinaryCrossentropy is not built for a conv net: use a softmax head with SparseCategoricalCrossentropy, or MeanSquaredError");
  if (m->dims[0] != s->F || m->max_batch != s->max_batch || m->max_p != s->max_p)
    return pyz_fail(PYZ_E_INVALID, "the Dense plan (input %d, max_batch %d, max_particles %d) does not continue the stem (%lld features, %d, %d)",
                    m->dims[0], m->max_batch, m->max_p, s->F, s->max_batch, s->max_p);
  return PYZ_OK;
}

inline const float *stem_features(const pyz_stem *s) { return s->op[s->n_ops - 1].out; }

// stem + Dense forward over the Dense layers [0, l_end) (all of them by default); the Dense outputs land in m->act
void convnet_forward(pyz_stem *s, pyz_mlp *m, const float *theta, int P, const float *x, const int32_t *row_idx, int batch,
                     hipStream_t st, int l_end = -1) {
  const long long Dt = s->D + m->D;
  stem_forward(s, theta, Dt, P, x, row_idx, batch, st);
  launch_forward(m, theta + s->D, Dt, P, stem_features(s), nullptr, batch, m->ctl, st, nullptr, l_end, nullptr, 0,
                 (long long)s->max_batch * s->F);
}

// forward, loss and (grad != null) the gradient of the whole vector into grad (P, D_total).  The callers have set the plan's
// ctl with set_ctl(..., row_off = 0, ...), and that zero matters: the stem's kernels read row_idx[b] as it stands, k_loss_*
// read row_idx[ctl->row_off + m] -- the images and the labels are the same rows only while row_off is 0 (a chained run,
// which moves row_off, would have to hand the stem row_idx + row_off)
int convnet_loss_backward(pyz_stem *s, pyz_mlp *m, const float *theta, int P, const float *x, const void *y,
                          const int32_t *row_idx, int batch, float *grad, hipStream_t st) {
  const long long Dt = s->D + m->D;
  convnet_forward(s, m, theta, P, x, row_idx, batch, st);
  launch_loss(m, P, y, row_idx, batch, m->ctl, grad != nullptr, st);   // the labels go through row_idx; the features are in batch order
  m->cur_nblk = loss_nblk(m, batch);
  if (!grad) return PYZ_OK;
  const StemOp &last = s->op[s->n_ops - 1];
  // (nothing has updated a weight by the time the feature gradient reads layer 0's: the updates are the callers' last launch)
  const TailOf tail{(long long)s->max_batch * s->F, Dt, last.delta, last.kind == PYZ_STEM_CONV ? last.act : PYZ_ACT_LINEAR};
  launch_backward(m, theta + s->D, Dt, P, stem_features(s), nullptr, batch, m->ctl, grad + s->D, st, nullptr, &tail);
  stem_backward(s, theta, Dt, P, x, row_idx, batch, grad, Dt, st);
  return PYZ_OK;
}

// ---------------------------------------------------------------- what the forward and read-out entries share
// A Dense model (s == nullptr) or a conv stem in front of a Dense tail.
struct Net {
  pyz_stem *s;
  pyz_mlp *m;
  long long D() const { return s ? s->D + m->D : m->D; }   // one row of weights
  // the forward of P rows of weights, stopping before Dense layer `upto` (all layers by default); outputs land in m->act
  void forward(const float *theta, int P, const float *x, const int32_t *row_idx, int batch, hipStream_t st, int upto = -1) const {
    if (s)
      convnet_forward(s, m, theta, P, x, row_idx, batch, st, upto);
    else
      launch_forward(m, theta, m->D, P, x, row_idx, batch, m->ctl, st, nullptr, upto);
  }
};

// The walk of every read-out over its draws, `chunk` rows of weights at a time: the forward of a chunk on the n rows of x (up
// to Dense layer `upto`; none with do_forward = false, where the epilogue runs a forward of its own), then
// epilogue(s0, S, weights of the chunk) -> code.  The caller has set the plan's ctl for n rows.
template <class Epilogue>
int for_draw_chunks(const Net &net, const float *weights, int n_samples, const float *x, int n, int chunk, hipStream_t st,
                    Epilogue &&epilogue, bool do_forward = true, int upto = -1) {
  for (int s0 = 0; s0 < n_samples; s0 += chunk) {
    const int S = std::min(chunk, n_samples - s0);
    const float *w = weights + (long long)s0 * net.D();
    if (do_forward) net.forward(w, S, x, nullptr, n, st, upto);
    const int rc = epilogue(s0, S, w);
    if (rc) return rc;
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// pyz_mlp_forward / pyz_convnet_forward behind their plan checks
int net_forward(const Net &net, const float *d_theta, int P, const float *d_x, const int32_t *d_row_idx, int batch,
                float *d_out, void *stream) {
  pyz_mlp *m = net.m;
  if (!d_theta || !d_x || !d_out) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  hipStream_t st = as_stream(stream);
  int rc = set_ctl(m, 0, batch, 0.0f, 0, 0, 0, st);
  if (rc) return rc;
  net.forward(d_theta, P, d_x, d_row_idx, batch, st);
  const int C = m->dims[m->L];
  PYZ_LAUNCH(k_forward_finish, dim3(cdiv(batch, 256), P), dim3(256), 0, st, m->act[m->L - 1], (long long)m->max_batch * C, C,
             m->acts[m->L - 1] == PYZ_ACT_SOFTMAX ? 1 : 0, batch, d_out);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// pyz_predict / pyz_convnet_predict (d_m2 == null) behind their argument checks
int net_predict(const Net &net, const float *d_weights, int n_samples, const float *d_x, int n, float *d_samples,
                float *d_mean, void *stream) {
  pyz_mlp *m = net.m;
  hipStream_t st = as_stream(stream);
  int rc = set_ctl(m, 0, n, 0.0f, 0, 0, 0, st);
  if (rc) return rc;
  const int C = m->dims[m->L];
  const int softmax = m->acts[m->L - 1] == PYZ_ACT_SOFTMAX ? 1 : 0;
  return for_draw_chunks(net, d_weights, n_samples, d_x, n, m->max_p, st, [&](int s0, int S, const float *) {
    PYZ_LAUNCH(k_predict_rows, dim3(cdiv(n, 256), S), dim3(256), 0, st, m->act[m->L - 1], (long long)m->max_batch * C, C,
               softmax, n, d_samples ? d_samples + (long long)s0 * n * C : nullptr);
    PYZ_LAUNCH(k_predict_mean, dim3((unsigned)cdiv((long long)n * C, 256)), dim3(256), 0, st, m->act[m->L - 1],
               (long long)m->max_batch * C, (long long)n * C, S, d_mean, s0 > 0 ? 1 : 0, 1.0f / (float)n_samples);
    return PYZ_OK;
  });
}

// pyz_predict_moments / pyz_convnet_predict (d_m2 != null) behind their argument checks
int net_predict_moments(const Net &net, const float *d_weights, int n_samples, const float *d_x, int n, float *d_mean,
                        float *d_m2, void *stream) {
  pyz_mlp *m = net.m;
  hipStream_t st = as_stream(stream);
  int rc = set_ctl(m, 0, n, 0.0f, 0, 0, 0, st);
  if (rc) return rc;
  PredictMomentsArgs g{};
  g.last = m->act[m->L - 1];
  g.C = m->dims[m->L];
  g.pstride = (long long)m->max_batch * g.C;
  g.softmax = m->acts[m->L - 1] == PYZ_ACT_SOFTMAX ? 1 : 0;
  g.n = n;
  g.mean = d_mean;
  g.m2 = d_m2;
  g.inv_total = 1.0f / (float)n_samples;
  return for_draw_chunks(net, d_weights, n_samples, d_x, n, m->max_p, st, [&](int s0, int S, const float *) {
    g.S = S;
    g.accumulate = s0 > 0 ? 1 : 0;
    if (!pyz_launch_predict_moments(g, st))
      return pyz_fail(PYZ_E_SHAPE, "a row of %d outputs does not fit the moments kernel's LDS", g.C);
    return PYZ_OK;
  });
}

}  // namespace

extern "C" {

int pyz_version(void) { return PYZ_VERSION; }

const char *pyz_last_error(void) { return pyz_err_slot().c_str(); }

int pyz_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pyz_mlp_create(int n_layers, const int32_t *h_dims, const int32_t *h_acts, int loss, int max_batch,
                   int max_particles, pyz_mlp **out) {
  if (!out || !h_dims || !h_acts) return pyz_fail(PYZ_E_INVALID, "null argument");
  *out = nullptr;
  if (n_layers < 1 || n_layers > PYZ_MAX_LAYERS) return pyz_fail(PYZ_E_INVALID, "n_layers %d outside [1, %d]", n_layers, PYZ_MAX_LAYERS);
  if (max_batch < 1 || max_particles < 1) return pyz_fail(PYZ_E_INVALID, "max_batch and max_particles must be >= 1");
  if (max_particles > 65535) return pyz_fail(PYZ_E_INVALID, "max_particles %d > 65535", max_particles);
  if (loss != PYZ_LOSS_SCCE && loss != PYZ_LOSS_MSE && loss != PYZ_LOSS_BCE) return pyz_fail(PYZ_E_INVALID, "unknown loss %d", loss);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return pyz_fail(PYZ_E_NODEV, "no HIP device visible");
  pyz_mlp_full *m = new pyz_mlp_full();
  m->L = n_layers;
  m->loss = loss;
  m->max_batch = max_batch;
  m->max_p = max_particles;
  long long off = 0;
  for (int l = 0; l <= n_layers; ++l) {
    if (h_dims[l] < 1) {
      delete m;
      return pyz_fail(PYZ_E_INVALID, "dims[%d] = %d", l, h_dims[l]);
    }
    m->dims[l] = h_dims[l];
  }
  for (int l = 0; l < n_layers; ++l) {
    const int a = h_acts[l];
    if (a < PYZ_ACT_LINEAR || a > PYZ_ACT_SOFTMAX || (a == PYZ_ACT_SOFTMAX && l != n_layers - 1)) {
      delete m;
      return pyz_fail(PYZ_E_INVALID, "activation %d at layer %d is not supported", a, l);
    }
    m->acts[l] = a;
    m->w_off[l] = off;
    off += (long long)(m->dims[l] + 1) * m->dims[l + 1];
  }
  m->D = off;
  // the kernels read a BinaryCrossentropy target as ONE float per row: a plan of any other shape is refused here, for
  // every entry point at once (the other two losses keep their per-call check: plans that only predict may carry any)
  if (loss == PYZ_LOSS_BCE) {
    const int rc = check_loss_combo(m);
    if (rc != PYZ_OK) {
      delete m;
      return rc;
    }
  }
  {  // the kernels address operands with 32-bit byte offsets from per-layer bases (buffer descriptors)
    long long widest = 0;
    for (int l = 0; l <= n_layers; ++l) widest = std::max<long long>(widest, m->dims[l]);
    if ((long long)max_batch * widest * 4 >= (1LL << 31) || off * 4 >= (1LL << 31)) {
      delete m;
      return pyz_fail(PYZ_E_INVALID, "max_batch x widest layer, or the parameter vector, exceeds 2 GiB");
    }
  }
  auto fail = [&](int rc) {
    pyz_mlp_destroy(m);
    return rc;
  };
  for (int l = 0; l < n_layers; ++l) {
    const size_t bytes = sizeof(float) * (size_t)max_particles * max_batch * m->dims[l + 1] + 64;
    if (hipMalloc((void **)&m->act[l], bytes) != hipSuccess || hipMalloc((void **)&m->delta[l], bytes) != hipSuccess)
      return fail(pyz_fail(PYZ_E_OOM, "workspace allocation of %zu bytes failed", bytes));
    m->ws_bytes += 2 * bytes;
  }
  {
    // two contiguous batches: chained runs assemble step s + 1's rows in the one that step s does not read
    // (or, PYZ_BATCH_FRAG [1] and an input width the images exist for, two slots of images: frag_slot_floats)
    m->frag_on = pyz_env_int("PYZ_BATCH_FRAG", 1) != 0 && m->dims[0] % 8 == 0;
    size_t bytes = 2 * sizeof(float) * (size_t)max_batch * m->dims[0] + 64;
    if (m->frag_on) bytes = std::max(bytes, 2 * sizeof(float) * frag_slot_floats(m) + 64);
    if (hipMalloc((void **)&m->xb, bytes) != hipSuccess) return fail(pyz_fail(PYZ_E_OOM, "workspace allocation of %zu bytes failed", bytes));
    m->ws_bytes += bytes;
  }
  if (hipMalloc((void **)&m->nonfinite, 64) != hipSuccess || hipMemset(m->nonfinite, 0, 64) != hipSuccess)
    return fail(pyz_fail(PYZ_E_OOM, "counter allocation failed"));
  if (hipMalloc((void **)&m->ctl, 2 * sizeof(StepCtl)) != hipSuccess) return fail(pyz_fail(PYZ_E_OOM, "ctl allocation failed"));
  if (hipMemset(m->ctl, 0, 2 * sizeof(StepCtl)) != hipSuccess) return fail(pyz_fail(PYZ_E_HIP, "ctl memset failed"));
  const size_t scal = sizeof(float) * (size_t)(max_particles * 16 + 64);
  if (hipMalloc((void **)&m->scal, scal) != hipSuccess) return fail(pyz_fail(PYZ_E_OOM, "scalar allocation failed"));
  m->ws_bytes += scal;
  {
    const int rc = need_part(m, (size_t)max_particles * max_batch + 8);  // up to one loss partial per row (k_head_rows)
    if (rc != PYZ_OK) return fail(rc);
  }
  // a single chain's one hidden layer of <= 200 units (C2): room for the partial sums of the split-reduction forward
  // (only when the opt-in is set when the plan is created: PYZ_FWD_KSPLIT >= 2)
  if (m->L == 2 && m->dims[1] > 192 && m->dims[1] <= 200 && pyz_env_int("PYZ_FWD_KSPLIT", 0) >= 2) {
    const int rc = ensure_bytes(&m->x.fwd_part, &m->x.fwd_part_cap, sizeof(float) * (size_t)8 * max_batch * m->dims[1], m);
    if (rc != PYZ_OK) return fail(rc);
  }
  // kernels with more than 64 KB of dynamic LDS: the allowance is a per-device attribute of the function, set here for the
  // device this plan lives on (one process may drive several devices, each through plans of its own)
  {
    const int gs_lds = (int)pyz_svgd_gs_lds_bytes();
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_svgd_gs<false>), hipFuncAttributeMaxDynamicSharedMemorySize, gs_lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_svgd_gs<true>), hipFuncAttributeMaxDynamicSharedMemorySize, gs_lds) != hipSuccess)
      return fail(pyz_fail(PYZ_E_HIP, "hipFuncSetAttribute(k_svgd_gs) failed"));
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_svgd_gs_resident), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)pyz_svgd_gs_res_lds_bytes()) != hipSuccess)
      return fail(pyz_fail(PYZ_E_HIP, "hipFuncSetAttribute(k_svgd_gs_resident) failed"));
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_svgd_gs_resident2), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)pyz_svgd_gs_res_lds_bytes()) != hipSuccess)
      return fail(pyz_fail(PYZ_E_HIP, "hipFuncSetAttribute(k_svgd_gs_resident2) failed"));
    const int gr_lds = (int)pyz_svgd_gram_lds_bytes();
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_svgd_gram_tile<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, gr_lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_svgd_gram_tile<2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, gr_lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_svgd_gram_tile<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, gr_lds) != hipSuccess)
      return fail(pyz_fail(PYZ_E_HIP, "hipFuncSetAttribute(k_svgd_gram_tile) failed"));
  }
  *out = m;
  return PYZ_OK;
}

int pyz_mlp_destroy(pyz_mlp *mm) {
  if (!mm) return PYZ_OK;
  pyz_mlp_full *m = full(mm);
  m->graphs.drop();
  m->x.hm_graphs.drop();
  m->x.hmc_run_graphs.drop();
  m->x.adam_graphs.drop();
  for (int l = 0; l < PYZ_MAX_LAYERS; ++l) {
    if (m->act[l]) (void)hipFree(m->act[l]);
    if (m->delta[l]) (void)hipFree(m->delta[l]);
  }
  void *ptrs[] = {m->grad, m->grad2, m->qsave, m->part, m->x.part2, m->scal, m->ctl, m->tab_bs, m->xb, m->x.hm_buf, m->x.hm_res_buf, m->x.gs_res_buf, m->x.fwd_part, m->nonfinite, m->x.hr_buf, m->x.hr_tab, m->x.tab_bc, m->x.fsvi_buf};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  if (m->x.tab_host) {
    (void)hipHostFree(m->x.tab_host);
    for (auto &e : m->x.tab_ev) (void)hipEventDestroy(e);
  }
  if (m->x.up_host) {
    (void)hipHostFree(m->x.up_host);
    for (auto &e : m->x.up_ev) (void)hipEventDestroy(e);
  }
  if (m->x.hr_host) {
    (void)hipHostFree(m->x.hr_host);
    for (auto &e : m->x.hr_ev) (void)hipEventDestroy(e);
  }
  if (m->h_pinned) (void)hipHostFree(m->h_pinned);
  delete m;
  return PYZ_OK;
}

int64_t pyz_mlp_param_count(const pyz_mlp *m) { return m ? m->D : -1; }
int64_t pyz_mlp_workspace_bytes(const pyz_mlp *m) { return m ? (int64_t)m->ws_bytes : -1; }

// ---------------------------------------------------------------- G1
int pyz_mlp_forward(pyz_mlp *m, const float *d_theta, int P, const float *d_x, const int32_t *d_row_idx, int batch,
                    float *d_out, void *stream) {
  int rc = check_call(m, P, batch);
  if (rc) return rc;
  return net_forward(Net{nullptr, m}, d_theta, P, d_x, d_row_idx, batch, d_out, stream);
}

// ---------------------------------------------------------------- G1-G3
int pyz_mlp_loss_grad(pyz_mlp *m, const float *d_theta, int P, const float *d_x, const void *d_y,
                      const int32_t *d_row_idx, int batch, float *d_grad, float *d_loss, void *stream) {
  int rc = check_call(m, P, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  hipStream_t st = as_stream(stream);
  set_ctl_lazy(m, batch, 0.0f, 0);
  WgradArgs u{};
  u.mode = PYZ_UPD_NONE;
  u.grad = d_grad;
  u.grad_pstride = m->D;
  launch_loss_backward(m, d_theta, m->D, P, d_x, d_y, d_row_idx, batch, m->ctl, d_grad != nullptr, u, st);
  PYZ_LAUNCH(k_loss_finalize, dim3(P), dim3(64), 0, st, m->part, m->cur_nblk, m->ctl, d_loss, m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- S1
int pyz_sgd_step(pyz_mlp *m, float *d_theta, const float *d_x, const void *d_y, const int32_t *d_row_idx, int batch,
                 float lr, float *d_loss, void *stream) {
  int rc = check_call(m, 1, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  const bool fused = can_fuse(m);
  if (!fused && (rc = need_grad(m, 1))) return rc;
  hipStream_t st = as_stream(stream);
  set_ctl_lazy(m, batch, lr, 0);
  WgradArgs u{};
  if (fused) {  // the update runs in the epilogue of the weight-gradient kernel
    u.mode = PYZ_UPD_SGD;
    u.theta = d_theta;
    u.loss = d_loss;
  } else {
    u.mode = PYZ_UPD_NONE;
    u.grad = m->grad;
    u.grad_pstride = m->D;
  }
  launch_loss_backward(m, d_theta, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, u, st);
  if (!fused)
    PYZ_LAUNCH(k_sgd_update, dim3(cdiv(m->D, 256)), dim3(256), 0, st, d_theta, m->grad, m->D, m->ctl, m->part,
                       m->cur_nblk, d_loss, m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- ADAM (ADAM.py:42-86) / VADAM (VADAM.py:44-98)
int pyz_adam_step(pyz_mlp *m, float *d_theta, float *d_m, float *d_v, const float *d_x, const void *d_y,
                  const int32_t *d_row_idx, int batch, float lr, double beta_1, double beta_2, int64_t epoch,
                  float denom_eps, float decay, float *d_loss, void *stream) {
  int rc = check_call(m, 1, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_m || !d_v || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (epoch < 1) return pyz_fail(PYZ_E_INVALID, "epoch %lld < 1", (long long)epoch);
  if (!(beta_1 >= 0.0 && beta_1 < 1.0) || !(beta_2 >= 0.0 && beta_2 < 1.0))
    return pyz_fail(PYZ_E_INVALID, "beta_1 = %g, beta_2 = %g: both must lie in [0, 1)", beta_1, beta_2);
  const bool fused = can_fuse(m);
  if (!fused && ((rc = need_grad(m, 1)) || (rc = need_grad2(m, 1)))) return rc;
  hipStream_t st = as_stream(stream);
  set_ctl_lazy(m, batch, lr, 0);
  AdamArgs a{};
  a.w.mode = PYZ_UPD_NONE;
  a.m = d_m;
  a.v = d_v;
  a.a = adam_scalars(lr, beta_1, beta_2, epoch, denom_eps, decay);
  if (fused) {  // gradients, squared-gradient means and the update in one weight-gradient launch
    a.w.theta = d_theta;
    a.w.loss = d_loss;
  } else {
    a.w.grad = m->grad;
    a.w.grad_pstride = m->D;
  }
  launch_loss_backward(m, d_theta, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, a.w, st, -1, &a);
  if (!fused)
    PYZ_LAUNCH(k_adam_update, dim3(cdiv(m->D, 256)), dim3(256), 0, st, d_theta, d_m, d_v, m->grad, m->grad2, m->D, a.a,
               m->ctl, m->part, m->cur_nblk, d_loss, m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_vadam_perturb(pyz_mlp *m, float *d_theta, const float *d_v, float lam, float num_data, int64_t step, uint64_t seed,
                      const float *d_eps, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (!d_theta || !d_v) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (!(num_data > 0.0f)) return pyz_fail(PYZ_E_INVALID, "num_data = %g must be positive", (double)num_data);
  if (step < 0) return pyz_fail(PYZ_E_INVALID, "negative step");
  PYZ_LAUNCH(k_vadam_perturb, dim3(cdiv(cdiv(m->D, 4), 256)), dim3(256), 0, as_stream(stream), d_theta, d_v, m->D, lam,
             num_data, seed, (uint32_t)step, d_eps);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- BSAM (BSAM.py:46-119)
int pyz_bsam_step(pyz_mlp *m, float *d_theta, float *d_m, float *d_v, const float *d_x, const void *d_y,
                  const int32_t *d_row_idx, int batch, float lr, double beta_1, double beta_2, float lam, float rho,
                  float gam, float num_data, int64_t step, uint64_t seed, const float *d_eps, float *d_loss, void *stream) {
  int rc = check_call(m, 1, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_m || !d_v || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (!(beta_1 >= 0.0 && beta_1 < 1.0) || !(beta_2 >= 0.0 && beta_2 < 1.0))
    return pyz_fail(PYZ_E_INVALID, "beta_1 = %g, beta_2 = %g: both must lie in [0, 1)", beta_1, beta_2);
  if (!(num_data > 0.0f)) return pyz_fail(PYZ_E_INVALID, "num_data = %g must be positive", (double)num_data);
  if (step < 0) return pyz_fail(PYZ_E_INVALID, "negative step");
  const bool fused = can_fuse(m);
  if ((rc = need_grad2(m, 1)) || (!fused && (rc = need_grad(m, 1)))) return rc;   // grad2 keeps the first pass's gradient
  hipStream_t st = as_stream(stream);
  BsamArgs a{};
  a.w.mode = PYZ_UPD_NONE;
  a.m = d_m;
  a.v = d_v;
  a.g1 = m->grad2;
  // each scalar in float64, rounded to float32 once (see BsamScal)
  a.a.lr = lr;
  a.a.b1 = (float)beta_1;
  a.a.c1 = (float)(1.0 - beta_1);
  a.a.b2 = (float)beta_2;
  a.a.c2 = (float)(1.0 - beta_2);
  a.a.lam = lam;
  a.a.rho = rho;
  a.a.gam = gam;
  a.a.inv_n = (float)(1.0 / (double)num_data);
  PYZ_LAUNCH(k_bsam_perturb, dim3(cdiv(cdiv(m->D, 4), 256)), dim3(256), 0, st, d_theta, d_v, m->D, a.a.inv_n, seed,
             (uint32_t)step, d_eps);
  set_ctl_lazy(m, batch, lr, 0);   // (carried by the first pass's first kernel; the second pass finds it in place)
  if (fused) {  // each pass ends in its weight-gradient launch: gradients + ascent, gradients + update
    a.w.theta = d_theta;
    a.w.loss = d_loss;
    launch_bsam_pass(m, d_theta, d_x, d_y, d_row_idx, batch, 0, a, st);
    a.w.loss = d_loss + 1;
    launch_bsam_pass(m, d_theta, d_x, d_y, d_row_idx, batch, 1, a, st);
  } else {
    a.w.grad = m->grad;
    a.w.grad_pstride = m->D;
    const dim3 grid(cdiv(m->D, 256)), block(256);
    launch_loss_backward(m, d_theta, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, a.w, st);
    PYZ_LAUNCH(k_bsam_ascent, grid, block, 0, st, d_theta, d_v, m->grad, m->grad2, m->D, a.a, m->ctl, m->part, m->cur_nblk,
               d_loss, m->nonfinite);
    launch_loss_backward(m, d_theta, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, a.w, st);
    PYZ_LAUNCH(k_bsam_update, grid, block, 0, st, d_theta, d_m, d_v, m->grad, m->grad2, m->D, a.a, m->ctl, m->part,
               m->cur_nblk, d_loss + 1, m->nonfinite);
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- FSVI (FSVI.py:60-147, DESIGN A8)
// what FSVI can run on, from the shape alone (no device is touched): FSVI.py:160-163 squeezes f[:, 0], :95 calls the loss
// with swapped arguments, and the D x D Stein system of :187-195 is dense
int pyz_fsvi_check(int n_layers, const int32_t *h_dims, const int32_t *h_acts, int loss, int k, int batch, int batch_size) {
  if (!h_dims || !h_acts) return pyz_fail(PYZ_E_INVALID, "null argument");
  if (n_layers < 1 || n_layers > PYZ_MAX_LAYERS) return pyz_fail(PYZ_E_INVALID, "n_layers %d outside [1, %d]", n_layers, PYZ_MAX_LAYERS);
  if (loss != PYZ_LOSS_MSE) return pyz_fail(PYZ_E_INVALID, "FSVI needs the MeanSquaredError loss (FSVI.py:95 swaps the loss's arguments)");
  if (h_acts[n_layers - 1] == PYZ_ACT_SOFTMAX) return pyz_fail(PYZ_E_INVALID, "FSVI does not take a softmax last layer");
  if (h_dims[n_layers] != 1)
    return pyz_fail(PYZ_E_INVALID, "FSVI needs a last layer of exactly one unit, not %d (FSVI.py:160 squeezes f[:, 0])", h_dims[n_layers]);
  if (k < 1) return pyz_fail(PYZ_E_INVALID, "FSVI needs k >= 1 particles, not %d", k);
  if (batch < 1 || batch_size < 1 || batch > batch_size)
    return pyz_fail(PYZ_E_INVALID, "batch %d outside [1, batch_size = %d]", batch, batch_size);
  if ((long long)batch + batch_size > PYZ_FSVI_MAX_N)
    return pyz_fail(PYZ_E_INVALID, "batch + measurement rows n = %lld exceed the limit of %d", (long long)batch + batch_size, PYZ_FSVI_MAX_N);
  long long D = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (h_dims[l] < 1) return pyz_fail(PYZ_E_INVALID, "dims[%d] = %d", l, h_dims[l]);
    D += (long long)(h_dims[l] + 1) * h_dims[l + 1];
  }
  if (D > PYZ_FSVI_MAX_D)
    return pyz_fail(PYZ_E_INVALID, "D = %lld weights exceed the limit of %d (the Stein system is D x D float64 per particle)", D, PYZ_FSVI_MAX_D);
  return PYZ_OK;
}

int pyz_spd_solve_f64(double *d_a, double *d_rhs, int n, int n_systems, int *d_fail, void *stream) {
  if (!d_a || !d_rhs) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n < 1 || n > PYZ_SPD_MAX_N) return pyz_fail(PYZ_E_INVALID, "system size %d outside [1, %d]", n, PYZ_SPD_MAX_N);
  if (n_systems < 1 || n_systems > 65535) return pyz_fail(PYZ_E_INVALID, "system count %d outside [1, 65535]", n_systems);
  int rc;
  if ((rc = pyz_spd_prepare())) return rc;
  pyz_launch_spd(d_a, d_rhs, n, n_systems, d_fail, as_stream(stream));
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_fsvi_step(pyz_mlp *m, float *d_mu, float *d_particles, int k, float *d_adam_m, float *d_adam_v, const float *d_x,
                  const float *d_y, const int32_t *d_row_idx, int batch, int batch_size, const float *d_lo, const float *d_hi,
                  float lr, int64_t t, uint64_t seed, const float *d_xm, const float *d_noise, const float *d_eps,
                  double *d_alpha, float *d_stein, float *d_grad, float *d_xp, float *d_f, float *d_loss, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  int rc;
  if ((rc = pyz_fsvi_check(m->L, m->dims, m->acts, m->loss, k, batch, batch_size))) return rc;
  const int n = batch + batch_size, F = m->dims[0];
  if ((rc = check_call(m, k, n))) return rc;   // the plan's rows hold batch + measurement rows
  if (!d_mu || !d_particles || !d_adam_m || !d_adam_v || !d_x || !d_y || !d_loss || (!d_xm && (!d_lo || !d_hi)))
    return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (t < 1 || t >= (1LL << 29)) return pyz_fail(PYZ_E_INVALID, "step t = %lld outside [1, 2^29)", (long long)t);
  const long long D = m->D;
  // workspace: allocated on the first call, grown when a call needs more, owned by the plan
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t o_xp = 0, o_gram = o_xp + up(sizeof(float) * (size_t)k * n * F),
               o_alpha = o_gram + up(sizeof(double) * (size_t)k * n * n), o_skm = o_alpha + up(sizeof(double) * (size_t)k * n),
               o_srhs = o_skm + up(sizeof(double) * (size_t)k * D * D), o_loss = o_srhs + up(sizeof(double) * (size_t)k * D),
               o_fail = o_loss + up(sizeof(double) * (size_t)k), total = o_fail + up(sizeof(int) * (size_t)2 * k);
  if ((rc = ensure_bytes(&full(m)->x.fsvi_buf, &full(m)->x.fsvi_cap, total, m))) return rc;
  if ((rc = need_grad(m, k))) return rc;
  if ((rc = pyz_spd_prepare())) return rc;
  unsigned char *ws = static_cast<unsigned char *>(full(m)->x.fsvi_buf);
  float *xp = d_xp ? d_xp : reinterpret_cast<float *>(ws + o_xp);
  double *gram = reinterpret_cast<double *>(ws + o_gram);
  double *alpha = d_alpha ? d_alpha : reinterpret_cast<double *>(ws + o_alpha);
  double *skm = reinterpret_cast<double *>(ws + o_skm), *srhs = reinterpret_cast<double *>(ws + o_srhs);
  double *loss_part = reinterpret_cast<double *>(ws + o_loss);
  int *fail = reinterpret_cast<int *>(ws + o_fail);
  hipStream_t st = as_stream(stream);
  if ((rc = set_ctl(m, 0, n, lr, t, 0, 0, st))) return rc;

  FsviInputs in{};                                   // FSVI.py:86-89, 106, 197-212
  in.x = d_x;
  in.row_idx = d_row_idx;
  in.lo = d_lo;
  in.hi = d_hi;
  in.xm = d_xm;
  in.noise = d_noise;
  in.xp = xp;
  in.k = k;
  in.b = batch;
  in.B = batch_size;
  in.F = F;
  in.seed = seed;
  in.t4 = (uint32_t)(4 * t);
  PYZ_LAUNCH(k_fsvi_inputs, dim3(cdiv((long long)k * n * F, 256)), dim3(256), 0, st, in);

  // the Stein system needs the particles only (FSVI.py:114)
  PYZ_LAUNCH(k_fsvi_stein_system, dim3((unsigned)D, k), dim3(256), 0, st, d_particles, (int)D, skm, srhs);
  pyz_launch_spd(skm, srhs, (int)D, k, fail + k, st);

  for (int l = 0; l < m->L; ++l) {                    // FSVI.py:108 (the forward of :91 gives the same batch rows)
    DenseArgs g = forward_args(m, l, d_particles, D, xp, nullptr, m->ctl, nullptr);
    if (l == 0) g.in_pstride = (long long)n * F;      // every particle has its own input rows
    g.wt = pyz_wt_for(k);
    pyz_launch_fwd(g, n, k, st);
  }
  const float *f = m->act[m->L - 1];
  PYZ_LAUNCH(k_fsvi_gram, dim3(cdiv((long long)n * n, 256), k), dim3(256), 0, st, xp, n, F, f, (long long)m->max_batch, gram, alpha, d_f);
  pyz_launch_spd(gram, alpha, n, k, fail, st);         // FSVI.py:160-163: d gp_ll / d f = -K^-1 f

  FsviDelta dg{};                                    // FSVI.py:95-98, 111
  const int l = m->L - 1;
  dg.f = f;
  dg.f_pstride = m->max_batch;
  dg.y = d_y;
  dg.row_idx = d_row_idx;
  dg.alpha = alpha;
  dg.delta_last = m->delta[l];
  dg.loss_part = loss_part;
  dg.H = m->dims[l];
  if (l > 0) {
    dg.h = m->act[l - 1];
    dg.h_pstride = (long long)m->max_batch * dg.H;
    dg.delta_prev = m->delta[l - 1];
    dg.act_prev = m->acts[l - 1];
  } else {
    dg.h = xp;
    dg.h_pstride = (long long)n * F;
    dg.delta_prev = nullptr;
  }
  dg.theta = d_particles;
  dg.grad = m->grad;
  dg.D = D;
  dg.w_off = m->w_off[l];
  dg.b = batch;
  dg.n = n;
  dg.act_last = m->acts[l];
  dg.cdat = (float)((double)k / (double)batch_size * 2.0 / (double)batch);   // FSVI.py:98: k / B with the hyperparameter B
  dg.inv_k = 1.0 / (double)k;
  PYZ_LAUNCH(k_fsvi_delta, dim3(k), dim3(256), 0, st, dg);

  launch_bwd_data_hidden(m, d_particles, D, k, n, m->ctl, st);   // delta[L-3 .. 0]
  for (int ll = m->L - 2; ll >= 0; --ll) {              // [dW; db] of the layers below the last
    DenseArgs g{};
    g.K = m->dims[ll];
    g.N = m->dims[ll + 1];
    if (ll == 0) {
      g.in = xp;
      g.in_pstride = (long long)n * F;
    } else {
      g.in = m->act[ll - 1];
      g.in_pstride = (long long)m->max_batch * g.K;
    }
    g.lda = g.K;
    g.aux = m->delta[ll];
    g.aux_pstride = (long long)m->max_batch * g.N;
    g.out = m->grad;
    g.out_pstride = D;
    g.w_off = m->w_off[ll];
    g.ctl = m->ctl;
    pyz_launch_bwd_weight(g, n, k, st);
  }

  FsviUpdate u{};                                    // FSVI.py:115-138, 228-231
  u.mu = d_mu;
  u.adam_m = d_adam_m;
  u.adam_v = d_adam_v;
  u.particles = d_particles;
  u.grad = m->grad;
  u.stein_sol = srhs;
  u.eps = d_eps;
  u.stein_out = d_stein;
  u.grad_out = d_grad;
  u.loss_part = loss_part;
  u.fail = fail;
  u.loss = d_loss;
  u.nonfinite = m->nonfinite;
  u.D = D;
  u.k = k;
  u.inv_k = (float)(1.0 / (double)k);
  u.lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow(0.999, (double)t)) / (1.0 - std::pow(0.9, (double)t)));
  u.seed = seed;
  u.t4 = (uint32_t)(4 * t);
  PYZ_LAUNCH(k_fsvi_update, dim3(cdiv(D, 256)), dim3(256), 0, st, u);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- SWAG (survey 8f, rank 2)
int pyz_swag_step(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev_row, const float *d_x,
                  const void *d_y, const int32_t *d_row_idx, int batch, float lr, int64_t n, int update_moments,
                  float *d_loss, void *stream) {
  int rc = check_call(m, 1, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_mean || !d_sq_mean || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n < 0) return pyz_fail(PYZ_E_INVALID, "negative step count");
  const bool fused = can_fuse(m);
  if (!fused && (rc = need_grad(m, 1))) return rc;
  hipStream_t st = as_stream(stream);
  set_ctl_lazy(m, batch, lr, n);
  WgradArgs u{};
  if (fused) {
    u.mode = PYZ_UPD_SWAG;
    u.theta = d_theta;
    u.mean = d_mean;
    u.sq_mean = d_sq_mean;
    u.dev_row = d_dev_row;
    u.swag_update = update_moments ? 1 : 0;
    u.loss = d_loss;
  } else {
    u.mode = PYZ_UPD_NONE;
    u.grad = m->grad;
    u.grad_pstride = m->D;
  }
  launch_loss_backward(m, d_theta, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, u, st);
  if (!fused)
    PYZ_LAUNCH(k_swag_update, dim3(cdiv(m->D, 256)), dim3(256), 0, st, d_theta, d_mean, d_sq_mean, d_dev_row,
                       m->grad, m->D, update_moments ? 1 : 0, m->ctl, m->part, m->cur_nblk, d_loss, m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- L2/L3
struct SwagChain {  // chained SWAG run: the (k, D) deviation matrix and the two hyper-parameters its bookkeeping needs
  float *dev;
  int k, freq;
};

struct BbbChain {  // chained BBB run: what the step needs beside mu (= theta), and the optional validation forward
  float *rho, *w;
  float *w2;                // sampling fused into the weight-gradient epilogue: the second weight buffer (steps on StepCtl slot 1), or nullptr
  float alpha, prior_mean, prior_rho;
  const float *pm_vec, *pr_vec;
  pyz_mlp *val;             // plan of the validation forward (max_batch >= n_val), or nullptr
  const float *val_x;
  const void *val_y;
  int n_val;
  float *val_losses;        // [slot] per step; written on the steps that validate (BBB.py:203: step % 10 != 0)
};

// per-run tables of the device-resident runs (n_tab entries: one padding entry, the last step prepares a slot nobody reads):
// batch sizes and learning rates share one device allocation; host_entry_bytes = what one entry takes in the pinned
// staging buffers (8; 16 with pyz_adam_run's bias-correction pairs)
static int ensure_run_tables(pyz_mlp *m, size_t n_tab, size_t host_entry_bytes, hipStream_t st) {
  pyz_mlp_full *f = full(m);
  if (m->tab_cap < (int)n_tab) {
    const size_t cap = std::max<size_t>(n_tab, 65536);  // generous: the table pointers are baked into the graphs
    if (m->tab_bs) PYZ_HIP(hipFree(m->tab_bs));
    m->tab_bs = nullptr;
    m->tab_lr = nullptr;
    PYZ_HIP(hipMalloc((void **)&m->tab_bs, 8 * cap));
    m->tab_lr = reinterpret_cast<float *>(m->tab_bs + cap);
    m->tab_cap = (int)cap;
    m->graphs.drop();
  }
  // the tables go up through two pinned buffers used in turn: a buffer is rewritten once the copy of the run
  // before the previous one has left it (no stream-wide synchronisation per call)
  if (f->x.tab_host_cap < host_entry_bytes * n_tab) {
    if (f->x.tab_host) {
      PYZ_HIP(hipStreamSynchronize(st));
      PYZ_HIP(hipHostFree(f->x.tab_host));
      f->x.tab_host = nullptr;
    } else {
      for (auto &e : f->x.tab_ev) PYZ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const size_t cap = std::max<size_t>(host_entry_bytes * n_tab, host_entry_bytes * 4096);
    PYZ_HIP(hipHostMalloc(&f->x.tab_host, 2 * cap));
    f->x.tab_host_cap = cap;
    f->x.tab_count = 0;
  }
  return PYZ_OK;
}

// What every run entry checks of its step count, its first slot and its batch sizes (h_epochs: the epoch counts of an ADAM /
// VADAM run, checked step by step beside them).  Returns the largest batch of the call, or the error.
// h_batch_sizes == nullptr: the first two checks alone, for an entry whose own checks stand between them and the third.
static int check_run(const pyz_mlp *m, int n_steps, int64_t slot0, const int32_t *h_batch_sizes, const int64_t *h_epochs = nullptr) {
  if (n_steps <= 0) return pyz_fail(PYZ_E_INVALID, "n_steps must be positive");
  if (slot0 < 0 || slot0 + n_steps > 0x7fffffff) return pyz_fail(PYZ_E_INVALID, "slot0 out of range");
  int bmax = 0;
  for (int s = 0; h_batch_sizes && s < n_steps; ++s) {
    if (h_batch_sizes[s] <= 0 || h_batch_sizes[s] > m->max_batch)
      return pyz_fail(PYZ_E_SHAPE, "batch size %d of step %d outside [1, %d]", h_batch_sizes[s], s, m->max_batch);
    if (h_epochs && h_epochs[s] < 1) return pyz_fail(PYZ_E_INVALID, "epoch %lld of step %d < 1", (long long)h_epochs[s], s);
    bmax = std::max(bmax, h_batch_sizes[s]);
  }
  return bmax;
}

// 1 - beta^epoch of every step of an ADAM / VADAM run, exactly as adam_scalars evaluates it for the eager step: the third table
struct RunBc {
  double beta_1, beta_2;
  const int64_t *h_epochs;
  float2 of(int s) const {
    const AdamScal a = adam_scalars(0.0f, beta_1, beta_2, h_epochs[s], 0.0f, 0.0f);
    return make_float2(a.bc1, a.bc2);
  }
};

// Sends up the per-run tables (one padding entry: the last step prepares a slot nobody reads; with bc, the bias-correction
// pairs beside batch sizes and learning rates) and sets the scalars of the first step.  ahead_batch > 0: the run assembles
// its batches one step ahead, and the first one goes out here, placed for the forward tiles of a batch of ahead_batch rows.
static int upload_run_tables(pyz_mlp *m, const int32_t *h_batch_sizes, const float *h_lr, int n_steps, int64_t n0, int64_t slot0,
                             const RunBc *bc, const float *d_x, const int32_t *d_row_idx, int ahead_batch, hipStream_t st) {
  Extra &x = full(m)->x;
  const bool frag = m->frag_next && ahead_batch;   // (set by sgld_run_impl for the call it is about to make; every other run: rows)
  m->frag_next = false;
  m->run_batch_form = ahead_batch ? (frag ? 2 : 1) : 0;
  int rc;
  const size_t n_tab = (size_t)n_steps + 1;
  if ((rc = ensure_run_tables(m, n_tab, bc ? 16 : 8, st))) return rc;
  if (bc && x.tab_bc_cap < m->tab_cap) {   // (as large as the other tables: its address is baked into the graphs too)
    if (x.tab_bc) PYZ_HIP(hipFree(x.tab_bc));
    x.tab_bc = nullptr;
    x.tab_bc_cap = 0;
    PYZ_HIP(hipMalloc((void **)&x.tab_bc, sizeof(float2) * (size_t)m->tab_cap));
    x.tab_bc_cap = m->tab_cap;
  }
  const long long row_stride = m->max_batch;
  m->pend_on = false;
  if (n_steps <= PYZ_INLINE_TAB) {
    // short run: the tables ride in the arguments of the launch that sets the first step's scalars
    InlineTabs tabs{};
    InlineBc ibc{};
    for (int s = 0; s < n_steps; ++s) {
      tabs.bs[s] = h_batch_sizes[s];
      tabs.lr[s] = h_lr[s];
    }
    tabs.bs[n_steps] = h_batch_sizes[n_steps - 1];
    tabs.lr[n_steps] = h_lr[n_steps - 1];
    tabs.n = n_steps + 1;
    for (int s = 0; bc && s <= n_steps; ++s) ibc.bc[s] = bc->of(std::min(s, n_steps - 1));
    if (ahead_batch) {   // ... together with the first batch of the run
      const PrepArgs pa = prep_args(m, d_x, d_row_idx, ahead_batch, row_stride, 0);
      if (frag) PYZ_LAUNCH_AS(k_run_start, k_run_start_frag, dim3(256), dim3(256), 0, st, m->ctl, tabs, m->tab_bs, m->tab_lr, (long long)n0, slot0 * row_stride, (int)slot0, frag_prep(m, pa, 0));
      else if (bc) PYZ_LAUNCH(k_run_start_bc, dim3(256), dim3(256), 0, st, m->ctl, tabs, ibc, m->tab_bs, m->tab_lr, x.tab_bc, (long long)n0, slot0 * row_stride, (int)slot0, pa);
      else PYZ_LAUNCH(k_run_start, dim3(256), dim3(256), 0, st, m->ctl, tabs, m->tab_bs, m->tab_lr, (long long)n0, slot0 * row_stride, (int)slot0, pa);
    } else {
      if (bc) PYZ_LAUNCH(k_set_ctl_tabs_bc, dim3(1), dim3(64), 0, st, m->ctl, tabs, ibc, m->tab_bs, m->tab_lr, x.tab_bc, (long long)n0, slot0 * row_stride, (int)slot0);
      else PYZ_LAUNCH(k_set_ctl_tabs, dim3(1), dim3(64), 0, st, m->ctl, tabs, m->tab_bs, m->tab_lr, (long long)n0, slot0 * row_stride, (int)slot0);
    }
    return PYZ_OK;
  }
  const unsigned slot = (unsigned)(x.tab_count & 1);
  if (x.tab_count >= 2) PYZ_HIP(hipEventSynchronize(x.tab_ev[slot]));
  ++x.tab_count;
  int32_t *hb = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(x.tab_host) + slot * x.tab_host_cap);
  float *hl = reinterpret_cast<float *>(hb + n_tab);
  float2 *hc = reinterpret_cast<float2 *>(hl + n_tab);   // (8 n_tab bytes in: aligned)
  std::memcpy(hb, h_batch_sizes, sizeof(int32_t) * n_steps);
  std::memcpy(hl, h_lr, sizeof(float) * n_steps);
  hb[n_steps] = h_batch_sizes[n_steps - 1];
  hl[n_steps] = h_lr[n_steps - 1];
  for (int s = 0; bc && s <= n_steps; ++s) hc[s] = bc->of(std::min(s, n_steps - 1));
  PYZ_HIP(hipMemcpyAsync(m->tab_bs, hb, sizeof(int32_t) * n_tab, hipMemcpyHostToDevice, st));
  PYZ_HIP(hipMemcpyAsync(m->tab_lr, hl, sizeof(float) * n_tab, hipMemcpyHostToDevice, st));
  if (bc) PYZ_HIP(hipMemcpyAsync(x.tab_bc, hc, sizeof(float2) * n_tab, hipMemcpyHostToDevice, st));
  PYZ_HIP(hipEventRecord(x.tab_ev[slot], st));
  if ((rc = set_ctl(m, 0, h_batch_sizes[0], h_lr[0], n0, slot0 * row_stride, 0, st, (int)slot0, n_steps))) return rc;
  if (frag) {   // the first batch of the run as images
    PYZ_LAUNCH_AS(k_prep_batch, k_prep_batch_frag, dim3(256), dim3(256), 0, st, frag_prep(m, prep_args(m, d_x, d_row_idx, ahead_batch, row_stride, 0), 0), m->ctl);
    return PYZ_OK;
  }
  if (ahead_batch)   // the first batch of the run (every later one is assembled by the step before it)
    PYZ_LAUNCH(k_prep_batch, dim3(256), dim3(256), 0, st, prep_args(m, d_x, d_row_idx, ahead_batch, row_stride, 0), m->ctl);
  return PYZ_OK;
}

static void launch_sgld_step(pyz_mlp *m, float *theta, float *mean, float *sq, const float *x, const void *y,
                             const int32_t *row_idx, int grid_batch, int slot, bool chained, long long row_stride,
                             uint64_t seed, const float *unit_noise, float *loss, hipStream_t st, int mode = PYZ_UPD_SGLD,
                             const SwagChain *swag = nullptr, const BbbChain *bbb = nullptr, bool first = true) {
  const StepCtl *ctl = m->ctl + slot;
  const bool frag = chained && m->run_batch_form == 2;   // the run keeps its batches as images (upload_run_tables)
  if (bbb) {   // BBB.step (BBB.py:128-211) inside a device-resident run: scalars from StepCtl, cost into slot (slot0 + i)
    // Sampling fused (bbb->w2): the weights and the log q - log p partials of step i + 1 come out of step i's weight-gradient
    // epilogue, into the buffers of the other StepCtl slot; only the first step of a chunk launches k_bbb_sample (for a later
    // chunk it rewrites what the chunk before left: same Philox step, same mu / rho).
    const int nblk_sample = cdiv(cdiv(m->D, 4), 256), tiles = wgrad_tiles(m);
    const bool fuse = bbb->w2 != nullptr;
    const size_t kl_stride = (size_t)std::max(nblk_sample, tiles);
    double *kl_cur = full(m)->x.part2 + (fuse ? (size_t)slot * kl_stride : 0);
    double *kl_next = full(m)->x.part2 + (size_t)(slot ^ 1) * kl_stride;
    float *w_cur = (fuse && slot) ? bbb->w2 : bbb->w, *w_next = slot ? bbb->w : bbb->w2;
    const bool sample = !fuse || first;
    if (sample) {
      BbbArgs a{};
      a.mu = theta;
      a.rho = bbb->rho;
      a.w = w_cur;
      a.D = m->D;
      a.alpha = bbb->alpha;
      a.prior_mean = bbb->prior_mean;
      a.prior_rho = bbb->prior_rho;
      a.pm_vec = bbb->pm_vec;
      a.pr_vec = bbb->pr_vec;
      a.seed = seed;
      a.part_kl = kl_cur;
      a.nblk_kl = nblk_sample;
      a.ctl = ctl;
      a.chained = 1;
      PYZ_LAUNCH(k_bbb_sample, dim3(nblk_sample), dim3(256), 0, st, a);
    }
    WgradArgs u{};
    u.mode = PYZ_UPD_BBB;
    u.theta = theta;
    u.mean = bbb->rho;
    u.sq_mean = w_cur;
    u.seed = seed;
    u.alpha = bbb->alpha;
    u.prior_mean = bbb->prior_mean;
    u.prior_rho = bbb->prior_rho;
    u.pm_vec = bbb->pm_vec;
    u.pr_vec = bbb->pr_vec;
    u.bbb_chained = 1;
    u.part_kl = kl_cur;
    u.nblk_kl = sample ? nblk_sample : tiles;
    if (fuse) {
      u.w_next = w_next;
      u.part_kl_next = kl_next;
    }
    u.cost = loss;
    u.next = chained ? m->ctl + (slot ^ 1) : nullptr;
    u.tab_bs = m->tab_bs;
    u.tab_lr = m->tab_lr;
    u.row_stride = row_stride;
    const bool ahead = chained && batch_ahead(m, row_idx);
    if (ahead) u.prep = prep_args(m, x, row_idx, grid_batch, row_stride, slot ^ 1);
    if (ahead && frag) u.prep.dst = frag_buf(m, slot ^ 1);
    launch_loss_backward(m, w_cur, m->D, 1, x, y, row_idx, grid_batch, ctl, true, u, st, ahead ? slot : -1, nullptr, ahead && frag);
    if (bbb->val) {   // the validation split through the weights this step sampled; the launches do nothing on every tenth step
      pyz_mlp *v = bbb->val;
      launch_forward(v, w_cur, v->D, 1, bbb->val_x, nullptr, bbb->n_val, v->ctl, st, nullptr, v->L - 1, ctl, 10);
      launch_head(v, w_cur, v->D, 1, bbb->val_x, bbb->val_y, nullptr, bbb->n_val, v->ctl, false, st, ctl, 10);
      PYZ_LAUNCH(k_loss_finalize_gated, dim3(1), dim3(64), 0, st, v->part, v->cur_nblk, v->ctl, bbb->val_losses, v->nonfinite, ctl, 10);
    }
    return;
  }
  if (can_fuse(m)) {
    WgradArgs u{};
    u.mode = mode;  // PYZ_UPD_SGLD, or PYZ_UPD_SGD / PYZ_UPD_SWAG for the chained SGD / SWAG runs (fused path only)
    if (swag) {
      u.swag_freq = swag->freq;
      u.swag_k = swag->k;
      u.dev_base = swag->dev;
      u.dev_stride = m->D;
    }
    u.theta = theta;
    u.mean = mean;
    u.sq_mean = sq;
    u.seed = seed;
    u.unit_noise = unit_noise;
    u.loss = loss;
    u.loss_indexed = chained ? 1 : 0;
    u.next = chained ? m->ctl + (slot ^ 1) : nullptr;
    u.tab_bs = m->tab_bs;
    u.tab_lr = m->tab_lr;
    u.row_stride = row_stride;
    const bool ahead = chained && batch_ahead(m, row_idx);
    if (ahead) u.prep = prep_args(m, x, row_idx, grid_batch, row_stride, slot ^ 1);
    if (ahead && frag) u.prep.dst = frag_buf(m, slot ^ 1);
    launch_loss_backward(m, theta, m->D, 1, x, y, row_idx, grid_batch, ctl, true, u, st, ahead ? slot : -1, nullptr, ahead && frag);
    return;
  }
  WgradArgs u{};
  u.mode = PYZ_UPD_NONE;
  u.grad = m->grad;
  u.grad_pstride = m->D;
  launch_loss_backward(m, theta, m->D, 1, x, y, row_idx, grid_batch, ctl, true, u, st);
  SgldArgs a{};
  a.theta = theta;
  a.mean = mean;
  a.sq_mean = sq;
  a.grad = m->grad;
  a.D = m->D;
  a.ctl = ctl;
  a.next = chained ? m->ctl + (slot ^ 1) : nullptr;
  a.tab_bs = m->tab_bs;
  a.tab_lr = m->tab_lr;
  a.row_stride = row_stride;
  a.seed = seed;
  a.unit_noise = unit_noise;
  a.part = m->part;
  a.nblk = m->cur_nblk;
  a.loss = loss;
  a.loss_indexed = chained ? 1 : 0;
  a.nonfinite = m->nonfinite;
  PYZ_LAUNCH(k_sgld_update, dim3(cdiv(cdiv(m->D, 4), 256)), dim3(256), 0, st, a);
}

int pyz_sgld_step(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, const float *d_x, const void *d_y,
                  const int32_t *d_row_idx, int batch, float lr, int64_t n, uint64_t seed, const float *d_unit_noise,
                  float *d_loss, void *stream) {
  int rc = check_call(m, 1, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_mean || !d_sq_mean || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n < 0) return pyz_fail(PYZ_E_INVALID, "negative step count");
  if (!can_fuse(m) && (rc = need_grad(m, 1))) return rc;
  hipStream_t st = as_stream(stream);
  set_ctl_lazy(m, batch, lr, n);
  launch_sgld_step(m, d_theta, d_mean, d_sq_mean, d_x, d_y, d_row_idx, batch, 0, false, 0, seed, d_unit_noise, d_loss, st);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

static int sgld_run_impl(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, const float *d_x, const void *d_y,
                         const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr, int n_steps,
                         int64_t n0, int64_t slot0, uint64_t seed, float *d_losses, int use_graph, void *stream,
                         int mode = PYZ_UPD_SGLD, const SwagChain *swag = nullptr, const BbbChain *bbb = nullptr) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (mode != PYZ_UPD_SGLD && !can_fuse(m))
    return pyz_fail(PYZ_E_INVALID, "the chained SGD / SWAG runs need a last layer of at most 32 units");
  if (mode == PYZ_UPD_SGD) d_mean = d_sq_mean = d_theta;  // not touched in this mode
  int rc = check_loss_combo(m);
  if (rc) return rc;
  if ((rc = check_run(m, n_steps, slot0, nullptr)) < 0) return rc;
  if (!d_theta || !d_mean || !d_sq_mean || !d_x || !d_y || !d_row_idx || !h_batch_sizes || !h_lr || !d_losses)
    return pyz_fail(PYZ_E_INVALID, "null pointer");
  const int bmax = check_run(m, n_steps, slot0, h_batch_sizes);
  if (bmax < 0) return bmax;
  if (!can_fuse(m) && (rc = need_grad(m, 1))) return rc;
  hipStream_t st = as_stream(stream);
  BbbChain bbb_local{};
  if (bbb) {
    static const int fuse_sample = pyz_env_int("PYZ_BBB_FUSE_SAMPLE", 1);
    if ((rc = need_part2(m, 2 * (size_t)std::max(cdiv(cdiv(m->D, 4), 256), wgrad_tiles(m))))) return rc;
    if (fuse_sample) {   // the plan's gradient buffer (idle on the fused path) is the second weight buffer
      if ((rc = need_grad(m, 1))) return rc;
      bbb_local = *bbb;
      bbb_local.w2 = m->grad;
      bbb = &bbb_local;
    }
    if (bbb->val) {   // the validation plan's step scalars: its batch is the whole split, for every step of the run
      pyz_mlp *v = bbb->val;
      if (v->D != m->D || !can_fuse(v) || bbb->n_val < 1 || bbb->n_val > v->max_batch || !bbb->val_x || !bbb->val_y || !bbb->val_losses)
        return pyz_fail(PYZ_E_INVALID, "validation plan / split does not fit the model");
      if ((rc = set_ctl(v, 0, bbb->n_val, 0.0f, 0, 0, 0, st))) return rc;
    }
  }
  const long long row_stride = m->max_batch;
  // every step is launched for the largest batch of the call: the first batch is placed for its forward tiles too
  // ... and, where the step's kernels are the ones that read them, as images (the same answer for every step of the call)
  const bool frag = m->frag_next = batch_frag(m, d_theta, d_x, d_row_idx, bmax);
  if ((rc = upload_run_tables(m, h_batch_sizes, h_lr, n_steps, n0, slot0, nullptr, d_x, d_row_idx,
                              batch_ahead(m, d_row_idx) ? bmax : 0, st)))
    return rc;

  int s = 0;
  m->run_graph_steps = m->run_eager_steps = m->run_graph_launches = 0;
  m->graphs.begin_call();   // (an eager call captures nothing: pyz_sgld_run_info)
  // A run of ANY length is replayed from captured graphs: chunks of G steps (slot 0) and ONE graph for the
  // remainder, captured for its exact length and kept (the other slots, least recently used one replaced) -- a
  // caller that repeats its run lengths (train(n) again, bench.py's warm-up / timed pair) pays one capture per
  // length and afterwards one graph launch per chunk.  Every chunk starts on StepCtl slot 0: G is even (the
  // ping-pong returns to slot 0) and the remainder comes last.
  static const int G = std::min(128, std::max(2, pyz_env_int("PYZ_GRAPH_STEPS", 32) & ~1));
  if (use_graph && st != nullptr && !pyz_probe().on) {
    // everything baked into the graphs goes into the key
    unsigned long long key = 1469598103934665603ull;
    auto mix = [&](unsigned long long v) { key = (key ^ v) * 1099511628211ull; };
    mix((unsigned long long)(uintptr_t)d_theta); mix((unsigned long long)(uintptr_t)d_mean);
    mix((unsigned long long)(uintptr_t)d_sq_mean); mix((unsigned long long)(uintptr_t)d_x);
    mix((unsigned long long)(uintptr_t)d_y); mix((unsigned long long)(uintptr_t)d_row_idx);
    mix((unsigned long long)(uintptr_t)d_losses); mix(seed); mix((unsigned long long)bmax);
    mix((unsigned long long)(uintptr_t)m->tab_bs); mix((unsigned long long)G); mix((unsigned long long)mode);
    mix(frag ? 1ull : 0ull);
    // (not the stream: an instantiated graph launches on any stream, and a caller that takes a fresh stream per run --
    // torch hands them out of a pool -- would otherwise re-capture every graph on every call)
    if (swag) { mix((unsigned long long)(uintptr_t)swag->dev); mix((unsigned long long)swag->k); mix((unsigned long long)swag->freq); }
    if (bbb) {
      unsigned fb[3];
      memcpy(&fb[0], &bbb->alpha, 4); memcpy(&fb[1], &bbb->prior_mean, 4); memcpy(&fb[2], &bbb->prior_rho, 4);
      for (unsigned b : fb) mix(b);
      mix((unsigned long long)(uintptr_t)bbb->pm_vec); mix((unsigned long long)(uintptr_t)bbb->pr_vec);
      mix((unsigned long long)(uintptr_t)bbb->val); mix((unsigned long long)(uintptr_t)bbb->val_x); mix((unsigned long long)(uintptr_t)bbb->val_y);
      mix((unsigned long long)bbb->n_val); mix((unsigned long long)(uintptr_t)bbb->val_losses);
      mix((unsigned long long)(uintptr_t)bbb->w2); mix((unsigned long long)(uintptr_t)bbb->rho); mix((unsigned long long)(uintptr_t)full(m)->x.part2);
    }
    m->graphs.rekey(key);
    while (s < n_steps) {
      const int len = std::min(G, n_steps - s);
      const bool rest = len < G;   // the remainder: its own graph, by exact length in slots 1 ..; slot 0 holds the full chunk
      rc = m->graphs.launch(len, 0, rest ? 1 : 0, rest ? PYZ_GRAPH_CHUNKS : 1, st, [&] {
        for (int k = 0; k < len; ++k)
          launch_sgld_step(m, d_theta, d_mean, d_sq_mean, d_x, d_y, d_row_idx, bmax, k & 1, true, row_stride, seed,
                           nullptr, d_losses, st, mode, swag, bbb, k == 0);
        return PYZ_OK;
      });
      if (rc) return rc;
      s += len;
      m->run_graph_steps += len;
      ++m->run_graph_launches;
    }
  }
  for (; s < n_steps; ++s) {
    launch_sgld_step(m, d_theta, d_mean, d_sq_mean, d_x, d_y, d_row_idx, bmax, s & 1, true, row_stride, seed, nullptr,
                     d_losses, st, mode, swag, bbb, s == 0);
    ++m->run_eager_steps;
  }
  // fused sampling: the weights of the last step stand in the second buffer when it ran on StepCtl slot 1
  if (bbb && bbb->w2 && ((n_steps - 1) & 1))
    PYZ_HIP(hipMemcpyAsync(bbb->w, bbb->w2, sizeof(float) * (size_t)m->D, hipMemcpyDeviceToDevice, st));
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_sgld_run(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, const float *d_x, const void *d_y,
                 const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr, int n_steps, int64_t n0,
                 int64_t slot0, uint64_t seed, float *d_losses, int use_graph, void *stream) {
  return sgld_run_impl(m, d_theta, d_mean, d_sq_mean, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, n_steps, n0, slot0, seed,
                       d_losses, use_graph, stream);
}

// ---- SGLD, P chains per launch (pyz_sgld_chains.h).  One step = the particle-batched gradient pass of pyz_svgd_gradients
// (all chains on ONE batch, PYZ_UPD_NONE into the plan's (P, D) gradient buffer, per-particle losses in the plan's scalars)
// and k_sgld_update_chains behind it.  SGLD lanes (pyz_sgld_lanes.h) are the same step with a learning rate per lane and
// the seed seed + c * seed_stride: k_sgld_update_lanes stands where k_sgld_update_chains stands, nothing else differs.
// `lanes`: the P rows are lanes -- their host rates h_lr and seed_stride are checked as well, and at most PYZ_MAX_LANES go.
// `row`: what the P rows are called in the messages when they are neither ("member": pyz_members.h).
static int sgld_rows_check(const pyz_mlp *m, bool lanes, const void *theta, const void *mean, const void *sq, int P,
                           const void *x, const void *y, const void *h_lr, const void *losses, int64_t n, int seed_stride,
                           const char *row = nullptr) {
  if (!row) row = lanes ? "lane" : "chain";
  if (P < 1) return pyz_fail(PYZ_E_INVALID, "n_%ss %d: at least one %s", row, P, row);
  if (n < 0) return pyz_fail(PYZ_E_INVALID, "negative step count");
  if (lanes && seed_stride != 0 && seed_stride != 1)
    return pyz_fail(PYZ_E_INVALID, "seed_stride %d: 0 (one noise stream for every lane) or 1 (seed + lane)", seed_stride);
  if (!theta || !mean || !sq || !x || !y || (lanes && !h_lr) || !losses)
    return pyz_fail(PYZ_E_INVALID, lanes ? "null pointer" : "null device pointer");
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  const int most = lanes ? std::min(m->max_p, PYZ_MAX_LANES) : m->max_p;
  if (P > most)
    return pyz_fail(PYZ_E_SHAPE, "n_%ss %d outside [1, %d] of the plan%s", row, P, most, lanes ? " and the library" : "");
  return check_loss_combo(m);
}

// the update's launch fills the chip once: 8 workgroups of 256 threads per CU over all P rows (see pyz_sgld_chains.h)
static dim3 sgld_rows_grid(long long groups, int P) {
  const long long per_row = std::max<long long>(1, 8LL * pyz_cu_count() / P);
  return dim3((unsigned)std::min<long long>(cdiv(groups, 256), per_row), (unsigned)P);
}

// The third update kind of the rows step: SGD / SWAG members (pyz_members.h, k_members_update) instead of SGLD chains or lanes.
struct MembersUpdate {
  bool swag;          // SWAG rows (else SGD rows: sq and dev unused)
  float *dev;         // (P, k, D)
  int k;
  int freq;           // a run: hit steps and deviation columns follow from the count on the device
  int hit, col;       // an eager step: the caller's flag and column
};

// lane_lr: the P host rates of this step's lanes (k_sgld_update_lanes, seed + c * seed_stride), or nullptr for chains
// (k_sgld_update_chains: ctl->lr, seed + c); members: the rows are ensemble members (k_members_update: ctl->lr, no noise)
static void launch_sgld_rows_step(pyz_mlp *m, float *theta, float *mean, float *sq, int P, const float *x, const void *y,
                                  const int32_t *row_idx, int grid_batch, int slot, bool chained, long long row_stride,
                                  uint64_t seed, const float *lane_lr, int seed_stride, const float *unit_noise, float *loss,
                                  hipStream_t st, const MembersUpdate *members = nullptr) {
  const StepCtl *ctl = m->ctl + slot;
  WgradArgs u{};
  u.mode = PYZ_UPD_NONE;
  u.grad = m->grad;
  u.grad_pstride = m->D;
  const bool fused = can_fuse(m);
  if (fused) u.ploss = m->scal;      // per-particle losses in the weight-gradient launch (every particle's spare workgroup)
  launch_loss_backward(m, theta, m->D, P, x, y, row_idx, grid_batch, ctl, true, u, st);
  if (!fused) PYZ_LAUNCH(k_loss_finalize, dim3(P), dim3(64), 0, st, m->part, m->cur_nblk, ctl, m->scal, m->nonfinite);
  if (members) {
    MembersArgs g{};
    g.theta = theta;
    g.mean = mean;
    g.sq_mean = members->swag ? sq : nullptr;
    g.dev = members->swag ? members->dev : nullptr;
    g.grad = m->grad;
    g.D = m->D;
    g.grad_pstride = m->D;
    g.groups = (m->D + 3) / 4;
    g.ctl = ctl;
    g.next = chained ? m->ctl + (slot ^ 1) : nullptr;
    g.tab_bs = m->tab_bs;
    g.tab_lr = m->tab_lr;
    g.row_stride = row_stride;
    g.ploss = m->scal;
    g.loss = loss;
    g.loss_indexed = chained ? 1 : 0;
    g.swag = members->swag ? 1 : 0;
    g.k = members->k;
    g.freq = members->freq;
    g.hit = members->hit;
    g.col = members->col;
    PYZ_LAUNCH(k_members_update, sgld_rows_grid(g.groups, P), dim3(256), 0, st, g);
    return;
  }
  SgldChainsArgs a{};
  a.theta = theta;
  a.mean = mean;
  a.sq_mean = sq;
  a.grad = m->grad;
  a.D = m->D;
  a.grad_pstride = m->D;
  a.groups = (m->D + 3) / 4;
  a.ctl = ctl;
  a.next = chained ? m->ctl + (slot ^ 1) : nullptr;
  a.tab_bs = m->tab_bs;
  a.tab_lr = m->tab_lr;
  a.row_stride = row_stride;
  a.seed = seed;
  a.unit_noise = unit_noise;
  a.ploss = m->scal;
  a.loss = loss;
  a.loss_indexed = chained ? 1 : 0;
  const dim3 grid = sgld_rows_grid(a.groups, P);
  if (!lane_lr) {
    PYZ_LAUNCH(k_sgld_update_chains, grid, dim3(256), 0, st, a);
    return;
  }
  SgldLanesArgs l{};
  l.c = a;
  l.seed_stride = (unsigned)seed_stride;
  for (int c = 0; c < P; ++c) l.rates.lr[c] = lane_lr[c];
  PYZ_LAUNCH(k_sgld_update_lanes, grid, dim3(256), 0, st, l);
}

// One eager step of P chains (lane_lr == nullptr: every chain at lr) or of P lanes (lane c at lane_lr[c]; the StepCtl's
// rate is lane 0's, the update reads the launch's own).
static int sgld_rows_step(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, int P, const float *d_x,
                          const void *d_y, const int32_t *d_row_idx, int batch, float lr, const float *lane_lr, int64_t n,
                          uint64_t seed, int seed_stride, const float *d_unit_noise, float *d_loss, void *stream,
                          const MembersUpdate *members = nullptr) {
  int rc;
  if ((rc = check_call(m, P, batch))) return rc;
  if ((rc = need_grad(m, P))) return rc;
  hipStream_t st = as_stream(stream);
  set_ctl_lazy(m, batch, lr, n);   // the first kernel of the pass carries the step scalars
  launch_sgld_rows_step(m, d_theta, d_mean, d_sq_mean, P, d_x, d_y, d_row_idx, batch, 0, false, 0, seed, lane_lr, seed_stride,
                        d_unit_noise, d_loss, st, members);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_sgld_chains_step(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, int n_chains, const float *d_x,
                         const void *d_y, const int32_t *d_row_idx, int batch, float lr, int64_t n, uint64_t seed,
                         const float *d_unit_noise, float *d_loss, void *stream) {
  const int rc = sgld_rows_check(m, false, d_theta, d_mean, d_sq_mean, n_chains, d_x, d_y, nullptr, d_loss, n, 0);
  return rc ? rc : sgld_rows_step(m, d_theta, d_mean, d_sq_mean, n_chains, d_x, d_y, d_row_idx, batch, lr, nullptr, n, seed, 0,
                                  d_unit_noise, d_loss, stream);
}

int pyz_sgld_lanes_step(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, int n_lanes, const float *d_x,
                        const void *d_y, const int32_t *d_row_idx, int batch, const float *h_lr, int64_t n, uint64_t seed,
                        int seed_stride, const float *d_unit_noise, float *d_loss, void *stream) {
  const int rc = sgld_rows_check(m, true, d_theta, d_mean, d_sq_mean, n_lanes, d_x, d_y, h_lr, d_loss, n, seed_stride);
  return rc ? rc : sgld_rows_step(m, d_theta, d_mean, d_sq_mean, n_lanes, d_x, d_y, d_row_idx, batch, h_lr[0], h_lr, n, seed,
                                  seed_stride, d_unit_noise, d_loss, stream);
}

// The run enqueues its steps one after the other (no graph: use_graph is accepted and pyz_last_run_info reports every step
// as eager).  Each step is launched for ITS OWN batch size -- the host has the sizes -- so that its launches are those of
// pyz_sgld_chains_step, whose weight-gradient launch picks its waves from the batch it is launched for: that is what makes
// the run equal the step calls bit for bit on ragged batches.  The scalars the kernels read still come from the device
// tables (StepCtl ping-pong, advanced by the update kernel), so nothing waits for the host between two steps.
// Chains: h_lr holds n_steps rates, the device's rate table.  Lanes: h_lr is the host's (n_steps, P) table, row s rides in
// step s's launch, and the device's rate table gets lane 0's column (nobody reads it: it keeps the StepCtl meaningful).
static int sgld_rows_run(pyz_mlp *m, bool lanes, float *d_theta, float *d_mean, float *d_sq_mean, int P, const float *d_x,
                         const void *d_y, const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr,
                         int n_steps, int64_t n0, int64_t slot0, uint64_t seed, int seed_stride, float *d_losses,
                         void *stream, const MembersUpdate *members = nullptr) {
  int rc = sgld_rows_check(m, lanes, d_theta, d_mean, d_sq_mean, P, d_x, d_y, h_lr, d_losses, n0, seed_stride,
                           members ? "member" : nullptr);
  if (rc) return rc;
  if (!d_row_idx || !h_batch_sizes || !h_lr) return pyz_fail(PYZ_E_INVALID, "null pointer");
  if ((rc = check_run(m, n_steps, slot0, h_batch_sizes)) < 0) return rc;
  if ((rc = need_grad(m, P))) return rc;
  hipStream_t st = as_stream(stream);
  const long long row_stride = m->max_batch;
  std::vector<float> lane0;
  for (int s = 0; lanes && s < n_steps; ++s) lane0.push_back(h_lr[(size_t)s * P]);
  // the tables go up as pyz_sgld_run sends them; no batch is assembled ahead
  if ((rc = upload_run_tables(m, h_batch_sizes, lanes ? lane0.data() : h_lr, n_steps, n0, slot0, nullptr, d_x, d_row_idx, 0, st)))
    return rc;
  m->run_graph_steps = m->run_eager_steps = m->run_graph_launches = 0;
  for (int s = 0; s < n_steps; ++s) {
    launch_sgld_rows_step(m, d_theta, d_mean, d_sq_mean, P, d_x, d_y, d_row_idx, h_batch_sizes[s], s & 1, true, row_stride,
                          seed, lanes ? h_lr + (size_t)s * P : nullptr, seed_stride, nullptr, d_losses, st, members);
    ++m->run_eager_steps;
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_sgld_chains_run(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, int n_chains, const float *d_x,
                        const void *d_y, const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr,
                        int n_steps, int64_t n0, int64_t slot0, uint64_t seed, float *d_losses, int use_graph,
                        void *stream) {
  (void)use_graph;
  return sgld_rows_run(m, false, d_theta, d_mean, d_sq_mean, n_chains, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, n_steps, n0,
                       slot0, seed, 0, d_losses, stream);
}

int pyz_sgld_lanes_run(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, int n_lanes, const float *d_x,
                       const void *d_y, const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr,
                       int n_steps, int64_t n0, int64_t slot0, uint64_t seed, int seed_stride, float *d_losses,
                       void *stream) {
  return sgld_rows_run(m, true, d_theta, d_mean, d_sq_mean, n_lanes, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, n_steps, n0,
                       slot0, seed, seed_stride, d_losses, stream);
}

// ---- SGD / SWAG members (pyz_members.h): P ensemble members per launch.  The rows step of the SGLD chains above with
// k_members_update behind the gradient pass; checks, grid rule and run loop are the ones chains use, so a run equals the
// step calls bit for bit on ragged batches, and use_graph is accepted and reported eager, as there.
static int members_check(const MembersUpdate &u, int frequency, bool run) {
  if (run && frequency < 1) return pyz_fail(PYZ_E_INVALID, "frequency %d: at least 1", frequency);
  if (u.swag && u.k < 1) return pyz_fail(PYZ_E_INVALID, "k %d: at least one deviation column", u.k);
  if (u.swag && !u.dev) return pyz_fail(PYZ_E_INVALID, "null deviation pointer");
  if (u.swag && !run && u.col >= u.k) return pyz_fail(PYZ_E_INVALID, "deviation column %d outside the %d of a member", u.col, u.k);
  return PYZ_OK;
}

// SGD.py:42-84 for n_members models at once: theta <- theta - lr grad per member; with update_mean (the caller's
// n % frequency == 0) the member's row of d_mean receives the new weights (SGD.py:78-84).
int pyz_sgd_members_step(pyz_mlp *m, float *d_theta, float *d_mean, int n_members, const float *d_x, const void *d_y,
                         const int32_t *d_row_idx, int batch, float lr, int64_t n, int update_mean, float *d_loss,
                         void *stream) {
  const MembersUpdate u{false, nullptr, 0, 0, update_mean ? 1 : 0, -1};
  const int rc = sgld_rows_check(m, false, d_theta, d_mean, d_mean, n_members, d_x, d_y, nullptr, d_loss, n, 0, "member");
  return rc ? rc : sgld_rows_step(m, d_theta, d_mean, nullptr, n_members, d_x, d_y, d_row_idx, batch, lr, nullptr, n, 0, 0,
                                  nullptr, d_loss, stream, &u);
}

// The SGD train loop (SGD.py:42-84 inside Optimizer.py:121-134) of n_members models as one device-resident run: the hit
// steps follow from the count n0 + s on the device, so the run is not cut where the "mean" is taken.
int pyz_sgd_members_run(pyz_mlp *m, float *d_theta, float *d_mean, int n_members, int frequency, const float *d_x,
                        const void *d_y, const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr,
                        int n_steps, int64_t n0, int64_t slot0, float *d_losses, int use_graph, void *stream) {
  (void)use_graph;
  const MembersUpdate u{false, nullptr, 0, frequency, 0, -1};
  const int rc = members_check(u, frequency, true);
  return rc ? rc : sgld_rows_run(m, false, d_theta, d_mean, d_mean, n_members, d_x, d_y, d_row_idx, h_batch_sizes, h_lr,
                                 n_steps, n0, slot0, 0, 0, d_losses, stream, &u);
}

// SWAG.py:61-92 for n_members models at once: pyz_swag_step's update per member; with update_moments the member's moments
// move and theta - mean goes to column dev_col of the member's (k, D) block of d_dev (dev_col < 0: to no column, as
// pyz_swag_step's d_dev_row = NULL).
int pyz_swag_members_step(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev, int k, int n_members,
                          const float *d_x, const void *d_y, const int32_t *d_row_idx, int batch, float lr, int64_t n,
                          int update_moments, int dev_col, float *d_loss, void *stream) {
  const MembersUpdate u{true, d_dev, k, 0, update_moments ? 1 : 0, dev_col};
  int rc = members_check(u, 1, false);
  if (rc) return rc;
  rc = sgld_rows_check(m, false, d_theta, d_mean, d_sq_mean, n_members, d_x, d_y, nullptr, d_loss, n, 0, "member");
  return rc ? rc : sgld_rows_step(m, d_theta, d_mean, d_sq_mean, n_members, d_x, d_y, d_row_idx, batch, lr, nullptr, n, 0, 0,
                                  nullptr, d_loss, stream, &u);
}

// The SWAG train loop (SWAG.py:43-94 inside Optimizer.py:121-134) of n_members models as one device-resident run.  As in
// pyz_swag_run the bookkeeping follows from the step count on the device: the members must have started at count 0 with
// every step run, so the first step of a call cannot have a count below its slot.
int pyz_swag_members_run(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev, int k, int frequency,
                         int n_members, const float *d_x, const void *d_y, const int32_t *d_row_idx,
                         const int32_t *h_batch_sizes, const float *h_lr, int n_steps, int64_t n0, int64_t slot0,
                         float *d_losses, int use_graph, void *stream) {
  (void)use_graph;
  const MembersUpdate u{true, d_dev, k, frequency, 0, -1};
  const int rc = members_check(u, frequency, true);
  if (rc) return rc;
  if (n0 >= 0 && slot0 >= 0 && n0 < slot0)
    return pyz_fail(PYZ_E_INVALID, "count %lld below slot %lld: the members did not start at count 0", (long long)n0,
                    (long long)slot0);
  return sgld_rows_run(m, false, d_theta, d_mean, d_sq_mean, n_members, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, n_steps, n0,
                       slot0, 0, 0, d_losses, stream, &u);
}

// ---- the scores of SGLD lanes (pyz_sgld_lanes.h)
// The loss sum (and wrong rows) of every lane over n rows: one particle-batched forward per chunk of max_particles lanes,
// as pyz_predict, with the last layer left at its logits where the loss head starts from them (one sigmoid unit), and
// k_lane_scores over m->act[L - 1].
int pyz_lane_scores(pyz_mlp *m, const float *d_weights, int n_lanes, const float *d_x, const void *d_y, int n,
                    double *d_loss_sum, int64_t *d_errors, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (n_lanes < 1 || n < 1) return pyz_fail(PYZ_E_INVALID, "n_lanes and n must be positive");
  if (!d_weights || !d_x || !d_y || !d_loss_sum) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n > m->max_batch) return pyz_fail(PYZ_E_SHAPE, "n %d exceeds the plan's max_batch %d", n, m->max_batch);
  int rc = check_loss_combo(m);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  if ((rc = set_ctl(m, 0, n, 0.0f, 0, 0, 0, st))) return rc;
  const int L = m->L, nblk = cdiv(n, 256), S_max = std::min(m->max_p, n_lanes);
  // stream-ordered scratch, gone when the last chunk's kernel has read it: two partial rows and a ticket per lane of a chunk
  const size_t words = (size_t)S_max * nblk;
  unsigned long long *ws = nullptr;
  PYZ_HIP(hipMallocAsync((void **)&ws, sizeof(unsigned long long) * (2 * words + (size_t)(S_max + 1) / 2), st));
  LaneScoreArgs g{};
  g.last = m->act[L - 1];
  g.C = m->dims[L];
  g.pstride = (long long)m->max_batch * g.C;
  g.loss = m->loss;
  g.n = n;
  g.y = d_y;
  g.part = ws;
  g.epart = ws + words;
  g.ticket = reinterpret_cast<unsigned *>(ws + 2 * words);
  // the forward stops before the last layer: that one is launch_forward's launch with the activation left off where the
  // head takes the logit
  rc = for_draw_chunks(Net{nullptr, m}, d_weights, n_lanes, d_x, n, m->max_p, st, [&](int s0, int S, const float *w) {
    DenseArgs f = forward_args(m, L - 1, w, m->D, d_x, nullptr, m->ctl, nullptr);
    if (m->loss == PYZ_LOSS_BCE) f.act = PYZ_ACT_LINEAR;
    f.wt = pyz_wt_for(S);
    if (!pyz_launch_fwd_ring(f, n, S, st)) {
      if (!f.row_idx && !f.init_on && !f.gather_out) f.rows_cap = std::min(n, m->max_batch);
      pyz_launch_fwd(f, n, S, st);
    }
    PYZ_HIP(hipMemsetAsync(g.ticket, 0, sizeof(unsigned) * (size_t)S, st));
    g.loss_sum = d_loss_sum + s0;
    g.errors = d_errors ? reinterpret_cast<long long *>(d_errors) + s0 : nullptr;
    PYZ_LAUNCH(k_lane_scores, dim3((unsigned)nblk, (unsigned)S), dim3(256), 0, st, g);
    return PYZ_OK;
  }, true, L - 1);
  PYZ_HIP(hipFreeAsync(ws, st));   // (also after a failed chunk: the scratch is not left behind)
  return rc;
}

// The SGD train loop (SGD.py:42-69 inside Optimizer.py:121-134) as one device-resident run: the launch sequence
// of pyz_sgld_run with the plain update in the weight-gradient epilogue (no noise, no moments).
int pyz_sgd_run(pyz_mlp *m, float *d_theta, const float *d_x, const void *d_y, const int32_t *d_row_idx,
                const int32_t *h_batch_sizes, const float *h_lr, int n_steps, int64_t slot0, float *d_losses, int use_graph,
                void *stream) {
  return sgld_run_impl(m, d_theta, d_theta, d_theta, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, n_steps, 0, slot0, 0, d_losses,
                       use_graph, stream, PYZ_UPD_SGD);
}

// The SWAG train loop (SWAG.py:43-94 inside Optimizer.py:121-134) as one device-resident run.  The moment / deviation
// bookkeeping follows from the step count on the device: it must have started at count 0 with every step run.
int pyz_swag_run(pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev, int k, int frequency,
                 const float *d_x, const void *d_y, const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr,
                 int n_steps, int64_t n0, int64_t slot0, float *d_losses, int use_graph, void *stream) {
  if (!d_dev || k < 1 || frequency < 1) return pyz_fail(PYZ_E_INVALID, "bad deviation matrix / k / frequency");
  if (n0 < 0) return pyz_fail(PYZ_E_INVALID, "negative step count");
  const SwagChain sc{d_dev, k, frequency};
  return sgld_run_impl(m, d_theta, d_mean, d_sq_mean, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, n_steps, n0, slot0, 0, d_losses,
                       use_graph, stream, PYZ_UPD_SWAG, &sc);
}

// ---------------------------------------------------------------- B2-B4
int pyz_bbb_step(pyz_mlp *m, float *d_mu, float *d_rho, float *d_w, const float *d_x, const void *d_y,
                 const int32_t *d_row_idx, int batch, float lr, float alpha, float prior_mean, float prior_rho,
                 const float *d_prior_mean_vec, const float *d_prior_rho_vec, int64_t step, uint64_t seed,
                 const float *d_eps, float *d_cost, void *stream) {
  int rc = check_call(m, 1, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_mu || !d_rho || !d_w || !d_x || !d_y || !d_cost) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if ((rc = need_grad(m, 1))) return rc;
  const int nblk_kl = cdiv(cdiv(m->D, 4), 256);
  if ((rc = need_part2(m, nblk_kl))) return rc;
  hipStream_t st = as_stream(stream);
  set_ctl_lazy(m, batch, lr, step);
  BbbArgs a{};
  a.mu = d_mu;
  a.rho = d_rho;
  a.w = d_w;
  a.grad = m->grad;
  a.D = m->D;
  a.lr = lr;
  a.alpha = alpha;
  a.prior_mean = prior_mean;
  a.prior_rho = prior_rho;
  a.pm_vec = d_prior_mean_vec;
  a.pr_vec = d_prior_rho_vec;
  a.seed = seed;
  a.step = (uint32_t)step;
  a.eps = d_eps;
  a.part_kl = full(m)->x.part2;
  a.nblk_kl = nblk_kl;
  a.part_loss = m->part;
  a.nblk_loss = loss_nblk(m, batch);
  a.ctl = m->ctl;
  a.cost = d_cost;
  a.nonfinite = m->nonfinite;
  PYZ_LAUNCH(k_bbb_sample, dim3(nblk_kl), dim3(256), 0, st, a);
  WgradArgs u{};
  if (can_fuse(m)) {  // the mu / rho update runs in the epilogue of the weight-gradient kernel
    u.mode = PYZ_UPD_BBB;
    u.theta = d_mu;
    u.mean = d_rho;
    u.sq_mean = d_w;
    u.seed = seed;
    u.unit_noise = d_eps;
    u.alpha = alpha;
    u.prior_mean = prior_mean;
    u.prior_rho = prior_rho;
    u.bbb_lr = lr;
    u.pm_vec = d_prior_mean_vec;
    u.pr_vec = d_prior_rho_vec;
    u.bbb_step = (uint32_t)step;
    u.part_kl = full(m)->x.part2;
    u.nblk_kl = nblk_kl;
    u.cost = d_cost;
    launch_loss_backward(m, d_w, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, u, st);
  } else {
    u.mode = PYZ_UPD_NONE;
    u.grad = m->grad;
    u.grad_pstride = m->D;
    launch_loss_backward(m, d_w, m->D, 1, d_x, d_y, d_row_idx, batch, m->ctl, true, u, st);
    a.nblk_loss = m->cur_nblk;
    PYZ_LAUNCH(k_bbb_update, dim3(nblk_kl), dim3(256), 0, st, a);
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// The BBB train loop (BBB.py:128-211 inside Optimizer.py:121-134) as one device-resident run: per step the launch
// sequence of pyz_bbb_step with the step scalars on the device (learning rate from the table, Philox step = step0 + i),
// batches assembled one step ahead, the cost triple of step i in d_costs[4 (slot0 + i) ..], and -- with a validation
// plan -- the validation split forwarded through the weights the step sampled on the steps BBB.py:203 validates
// (step % 10 != 0; the launches are in every step of the graph and return at once on the others).
int pyz_bbb_run(pyz_mlp *m, float *d_mu, float *d_rho, float *d_w, const float *d_x, const void *d_y,
                const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr, int n_steps, float alpha,
                float prior_mean, float prior_rho, const float *d_prior_mean_vec, const float *d_prior_rho_vec, int64_t step0,
                int64_t slot0, uint64_t seed, float *d_costs, pyz_mlp *val_plan, const float *d_val_x, const void *d_val_y,
                int n_val, float *d_val_losses, int use_graph, void *stream) {
  if (!d_rho || !d_w) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (step0 < 0) return pyz_fail(PYZ_E_INVALID, "negative step count");
  BbbChain bc{};
  bc.rho = d_rho;
  bc.w = d_w;
  bc.alpha = alpha;
  bc.prior_mean = prior_mean;
  bc.prior_rho = prior_rho;
  bc.pm_vec = d_prior_mean_vec;
  bc.pr_vec = d_prior_rho_vec;
  bc.val = val_plan;
  bc.val_x = d_val_x;
  bc.val_y = d_val_y;
  bc.n_val = n_val;
  bc.val_losses = d_val_losses;
  return sgld_run_impl(m, d_mu, d_rho, d_w, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, n_steps, step0, slot0, seed, d_costs,
                       use_graph, stream, PYZ_UPD_BBB, nullptr, &bc);
}

// ---- BBB lanes (pyz_bbb_lanes.h): n_lanes posteriors that differ by lr, alpha and their scalar prior, as the rows of one
// particle-batched step.  Launch order: k_bbb_sample_lanes, the gradient pass of the SGLD rows step (PYZ_UPD_NONE into the
// plan's (P, D) gradient buffer, per-particle losses in the plan's scalars), k_loss_finalize when the head is not fused,
// k_bbb_update_lanes.
static int bbb_lanes_check(const pyz_mlp *m, const void *mu, const void *rho, const void *w, int P, const void *x, const void *y,
                           const void *h_lr, const void *h_alpha, const void *h_pm, const void *h_pr, const void *pm_vec,
                           const void *pr_vec, int64_t step, int seed_stride, const void *cost) {
  if (P < 1) return pyz_fail(PYZ_E_INVALID, "n_lanes %d: at least one lane", P);
  if (step < 0) return pyz_fail(PYZ_E_INVALID, "negative step count");
  if (seed_stride != 0 && seed_stride != 1)
    return pyz_fail(PYZ_E_INVALID, "seed_stride %d: 0 (one noise stream for every lane) or 1 (seed + lane)", seed_stride);
  if (!mu || !rho || !w || !x || !y || !h_lr || !h_alpha || !h_pm || !h_pr || !cost) return pyz_fail(PYZ_E_INVALID, "null pointer");
  if ((pm_vec == nullptr) != (pr_vec == nullptr))
    return pyz_fail(PYZ_E_INVALID, "prior vectors: both the mean and the rho vector, or neither");
  if (P > PYZ_MAX_LANES) return pyz_fail(PYZ_E_SHAPE, "n_lanes %d outside [1, %d] of the library", P, PYZ_MAX_LANES);
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (P > m->max_p) return pyz_fail(PYZ_E_SHAPE, "n_lanes %d outside [1, %d] of the plan", P, m->max_p);
  return check_loss_combo(m);
}

struct BbbLanes {   // what a lanes step needs beside the plan and the batch
  float *mu, *rho, *w;
  int P;
  const float *h_lr, *h_alpha, *h_pm, *h_pr;   // host, [P] each
  const float *pm_vec, *pr_vec;
  uint64_t seed;
  int seed_stride;
};

static void launch_bbb_lanes_step(pyz_mlp *m, const BbbLanes &b, const float *x, const void *y, const int32_t *row_idx,
                                  int grid_batch, int slot, bool chained, long long row_stride, int64_t step,
                                  const float *eps, float *cost, hipStream_t st) {
  const StepCtl *ctl = m->ctl + slot;
  const int P = b.P;
  BbbLanesArgs a{};
  a.mu = b.mu;
  a.rho = b.rho;
  a.w = b.w;
  a.grad = m->grad;
  a.D = m->D;
  a.grad_pstride = m->D;
  a.groups = (m->D + 3) / 4;
  a.nblk = cdiv(cdiv(m->D, 4), 256);
  a.pm_vec = b.pm_vec;
  a.pr_vec = b.pr_vec;
  a.seed = b.seed;
  a.seed_stride = (unsigned)b.seed_stride;
  a.step = (uint32_t)step;
  a.chained = chained ? 1 : 0;
  a.eps = eps;
  a.part_kl = full(m)->x.part2;
  a.ploss = m->scal;
  a.ctl = ctl;
  a.next = chained ? m->ctl + (slot ^ 1) : nullptr;
  a.tab_bs = m->tab_bs;
  a.tab_lr = m->tab_lr;
  a.row_stride = row_stride;
  a.cost = cost;
  a.nonfinite = m->nonfinite;
  for (int c = 0; c < P; ++c) {
    a.tab.lr[c] = b.h_lr[c];
    a.tab.alpha[c] = b.h_alpha[c];
    a.tab.prior_mean[c] = b.h_pm[c];
    a.tab.prior_rho[c] = b.h_pr[c];
  }
  const dim3 grid = sgld_rows_grid(a.groups, P);
  PYZ_LAUNCH(k_bbb_sample_lanes, grid, dim3(256), 0, st, a);
  WgradArgs u{};
  u.mode = PYZ_UPD_NONE;
  u.grad = m->grad;
  u.grad_pstride = m->D;
  const bool fused = can_fuse(m);
  if (fused) u.ploss = m->scal;
  launch_loss_backward(m, b.w, m->D, P, x, y, row_idx, grid_batch, ctl, true, u, st);
  if (!fused) PYZ_LAUNCH(k_loss_finalize, dim3(P), dim3(64), 0, st, m->part, m->cur_nblk, ctl, m->scal, m->nonfinite);
  PYZ_LAUNCH(k_bbb_update_lanes, grid, dim3(256), 0, st, a);
}

int pyz_bbb_lanes_step(pyz_mlp *m, float *d_mu, float *d_rho, float *d_w, int n_lanes, const float *d_x, const void *d_y,
                       const int32_t *d_row_idx, int batch, const float *h_lr, const float *h_alpha, const float *h_prior_mean,
                       const float *h_prior_rho, const float *d_prior_mean_vec, const float *d_prior_rho_vec, int64_t step,
                       uint64_t seed, int seed_stride, const float *d_eps, float *d_cost, void *stream) {
  int rc = bbb_lanes_check(m, d_mu, d_rho, d_w, n_lanes, d_x, d_y, h_lr, h_alpha, h_prior_mean, h_prior_rho, d_prior_mean_vec,
                           d_prior_rho_vec, step, seed_stride, d_cost);
  if (rc) return rc;
  if ((rc = check_call(m, n_lanes, batch))) return rc;
  if ((rc = need_grad(m, n_lanes))) return rc;
  if ((rc = need_part2(m, (size_t)n_lanes * cdiv(cdiv(m->D, 4), 256)))) return rc;
  hipStream_t st = as_stream(stream);
  set_ctl_lazy(m, batch, h_lr[0], step);   // the first kernel of the gradient pass carries the step scalars
  const BbbLanes b{d_mu, d_rho, d_w, n_lanes, h_lr, h_alpha, h_prior_mean, h_prior_rho, d_prior_mean_vec, d_prior_rho_vec,
                   seed, seed_stride};
  launch_bbb_lanes_step(m, b, d_x, d_y, d_row_idx, batch, 0, false, 0, step, d_eps, d_cost, st);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// The run on the skeleton of sgld_rows_run: every step enqueued for its own batch size (pyz_last_run_info reports eager
// steps), the StepCtl ping-pong advanced by lane 0 of the update kernel, nothing synchronises inside the call.  The
// lanes' numbers hold for every step of the call; the device's rate table gets lane 0's lr (nobody reads it).  There is
// no validation forward inside the run.
int pyz_bbb_lanes_run(pyz_mlp *m, float *d_mu, float *d_rho, float *d_w, int n_lanes, const float *d_x, const void *d_y,
                      const float *h_lr, const float *h_alpha, const float *h_prior_mean, const float *h_prior_rho,
                      const float *d_prior_mean_vec, const float *d_prior_rho_vec, const int32_t *d_row_idx,
                      const int32_t *h_batch_sizes, int n_steps, int64_t step0, int64_t slot0, uint64_t seed, int seed_stride,
                      float *d_costs, void *stream) {
  int rc = bbb_lanes_check(m, d_mu, d_rho, d_w, n_lanes, d_x, d_y, h_lr, h_alpha, h_prior_mean, h_prior_rho, d_prior_mean_vec,
                           d_prior_rho_vec, step0, seed_stride, d_costs);
  if (rc) return rc;
  if (!d_row_idx || !h_batch_sizes) return pyz_fail(PYZ_E_INVALID, "null pointer");
  if ((rc = check_run(m, n_steps, slot0, h_batch_sizes)) < 0) return rc;
  if ((rc = need_grad(m, n_lanes))) return rc;
  if ((rc = need_part2(m, (size_t)n_lanes * cdiv(cdiv(m->D, 4), 256)))) return rc;
  hipStream_t st = as_stream(stream);
  const long long row_stride = m->max_batch;
  const std::vector<float> lane0((size_t)n_steps, h_lr[0]);
  if ((rc = upload_run_tables(m, h_batch_sizes, lane0.data(), n_steps, step0, slot0, nullptr, d_x, d_row_idx, 0, st))) return rc;
  m->run_graph_steps = m->run_eager_steps = m->run_graph_launches = 0;
  const BbbLanes b{d_mu, d_rho, d_w, n_lanes, h_lr, h_alpha, h_prior_mean, h_prior_rho, d_prior_mean_vec, d_prior_rho_vec,
                   seed, seed_stride};
  for (int s = 0; s < n_steps; ++s) {
    launch_bbb_lanes_step(m, b, d_x, d_y, d_row_idx, h_batch_sizes[s], s & 1, true, row_stride, step0 + s, nullptr, d_costs, st);
    ++m->run_eager_steps;
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- ADAM / VADAM / BSAM train loops, device resident
// ADAM.step / VADAM.step / BSAM.step inside Optimizer.train (ADAM.py:42-86, VADAM.py:45-99, BSAM.py:46-119,
// Optimizer.py:121-134) as one device-resident run: sgld_run_impl's plumbing (StepCtl ping-pong, tab_bs / tab_lr, batches
// assembled one step ahead, graphs of PYZ_GRAPH_STEPS steps and one of the exact remaining length) around the launch
// sequence of pyz_adam_step / pyz_bsam_step, with the chained k_wgrad_adam / k_wgrad_bsam at the end of each pass.  Unlike the
// SGLD run every step is launched for its OWN batch size, not for the largest of the call: the wave count of the
// weight-gradient reduction (pyz_pick_waves) follows from it, and the results are to equal the eager steps bit for bit
// on the ragged last batch of an epoch too.  A graph therefore holds steps of one batch size and is kept by its length, that
// size and the StepCtl slot it starts on, in a cache of these runs' own (Extra::ar_*; the graphs of the other runs on the plan
// stay); a call of equal batches is chunked exactly as in sgld_run_impl.
struct AdamRunCfg {
  bool bsam;
  float *m, *v;
  AdamScal as;         // ADAM / VADAM (lr, bc1, bc2 come per step)
  BsamScal bs;         // BSAM (lr comes per step)
  RunChain c;          // c.perturb: the perturbation of step i + 1 rides in step i's epilogue
  bool perturbs;       // VADAM, BSAM
  uint64_t seed;
};

static void launch_wgrad_adam_run(pyz_mlp *m, const float *x, const int32_t *row_idx, int grid_batch, const StepCtl *ctl,
                                  AdamRunArgs &a, hipStream_t st, const float *gathered) {
  const int tiles = wgrad_layers(m, 1, x, row_idx, ctl, a.w, gathered);
  const int S = pyz_pick_waves(tiles, (grid_batch + 1) / 2);
  dim3 grid(tiles + 1);   // + the duties workgroup
  if (a.w.prep.src) grid.x = (unsigned)(tiles + 1 + std::max(pyz_cu_count() - tiles - 1, 24));  // + the batch workers
  switch (S) {
    case 1: PYZ_LAUNCH((k_wgrad_adam<1, true>), grid, dim3(64), 0, st, a); break;
    case 2: PYZ_LAUNCH((k_wgrad_adam<2, true>), grid, dim3(128), 2 * 4096, st, a); break;
    case 4: PYZ_LAUNCH((k_wgrad_adam<4, true>), grid, dim3(256), 4 * 4096, st, a); break;
    case 8: PYZ_LAUNCH((k_wgrad_adam<8, true>), grid, dim3(512), 8 * 4096, st, a); break;
    default: PYZ_LAUNCH((k_wgrad_adam<16, true>), grid, dim3(1024), 16 * 4096, st, a); break;
  }
}

static void launch_wgrad_bsam_run(pyz_mlp *m, const float *x, const int32_t *row_idx, int grid_batch, const StepCtl *ctl,
                                  int phase, BsamRunArgs &a, hipStream_t st, const float *gathered) {
  const int tiles = wgrad_layers(m, 1, x, row_idx, ctl, a.w, gathered);
  const int S = pyz_pick_waves(tiles, (grid_batch + 1) / 2);
  dim3 grid(tiles + 1);   // + the duties workgroup
  if (a.w.prep.src) grid.x = (unsigned)(tiles + 1 + std::max(pyz_cu_count() - tiles - 1, 24));  // + the batch workers
#define PYZ_BSAM_CASE(W, LDS)                                                               \
  if (phase == 0) PYZ_LAUNCH((k_wgrad_bsam<W, 0, true>), grid, dim3(64 * W), LDS, st, a);     \
  else PYZ_LAUNCH((k_wgrad_bsam<W, 1, true>), grid, dim3(64 * W), LDS, st, a);                \
  break
  switch (S) {
    case 1: PYZ_BSAM_CASE(1, 0);
    case 2: PYZ_BSAM_CASE(2, 2 * 4096);
    case 4: PYZ_BSAM_CASE(4, 4 * 4096);
    case 8: PYZ_BSAM_CASE(8, 8 * 4096);
    default: PYZ_BSAM_CASE(16, 16 * 4096);
  }
#undef PYZ_BSAM_CASE
}

// one step of the run on StepCtl slot `slot`, launched for its own batch size (the batch it assembles for the step behind it
// is placed for the forward tiles of a full batch: placement only changes speed)
static void launch_adam_run_step(pyz_mlp *m, const AdamRunCfg &c, float *theta, const float *x, const void *y,
                                 const int32_t *row_idx, int grid_batch, int slot, long long row_stride, float *losses,
                                 hipStream_t st) {
  const StepCtl *ctl = m->ctl + slot;
  const unsigned pgrid = (unsigned)cdiv(cdiv(m->D, 4), 256);
  if (c.perturbs && !c.c.perturb) {   // PYZ_ADAM_FUSE_PERTURB=0: the step's perturbation as a launch of its own
    if (c.bsam) PYZ_LAUNCH(k_bsam_perturb_run, dim3(pgrid), dim3(256), 0, st, theta, c.v, m->D, c.bs.inv_n, c.seed, ctl);
    else PYZ_LAUNCH(k_vadam_perturb_run, dim3(pgrid), dim3(256), 0, st, theta, c.v, m->D, c.c.lam, c.c.num_data, c.seed, ctl);
  }
  const bool ahead = batch_ahead(m, row_idx);
  static const int use_xb = pyz_env_int("PYZ_GATHER_COPY", 1);  // 1: forward leaves a contiguous batch copy
  for (int phase = 0; phase < (c.bsam ? 2 : 1); ++phase) {
    const float *rows;   // the contiguous rows of this step's batch that the weight-gradient kernel reads (or nullptr: gathered)
    if (ahead) {
      rows = batch_buf(m, slot);
      launch_forward(m, theta, m->D, 1, rows, nullptr, grid_batch, ctl, st, nullptr, m->L - 1);
    } else {
      float *xb = (use_xb && m->L > 1) ? m->xb : nullptr;
      rows = xb;
      launch_forward(m, theta, m->D, 1, x, row_idx, grid_batch, ctl, st, xb, m->L - 1);
    }
    launch_head(m, theta, m->D, 1, x, y, row_idx, grid_batch, ctl, true, st);   // (labels go through row_idx)
    launch_bwd_data_hidden(m, theta, m->D, 1, grid_batch, ctl, st);
    const bool last = phase == (c.bsam ? 1 : 0);
    WgradArgs w{};
    w.mode = PYZ_UPD_NONE;
    w.theta = theta;
    w.loss = losses;
    w.seed = c.seed;
    w.next = m->ctl + (slot ^ 1);
    w.tab_bs = m->tab_bs;
    w.tab_lr = m->tab_lr;
    w.row_stride = row_stride;
    if (ahead && last) w.prep = prep_args(m, x, row_idx, m->max_batch, row_stride, slot ^ 1);
    if (c.bsam) {
      BsamRunArgs a{};
      a.w = w;
      a.m = c.m;
      a.v = c.v;
      a.g1 = m->grad2;
      a.a = c.bs;
      a.c = c.c;
      launch_wgrad_bsam_run(m, x, row_idx, grid_batch, ctl, phase, a, st, rows);
    } else {
      AdamRunArgs a{};
      a.w = w;
      a.m = c.m;
      a.v = c.v;
      a.a = c.as;
      a.c = c.c;
      launch_wgrad_adam_run(m, x, row_idx, grid_batch, ctl, a, st, rows);
    }
  }
}

static int adam_run_impl(pyz_mlp *m, AdamRunCfg &c, float *d_theta, const float *d_x, const void *d_y,
                         const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr, const int64_t *h_epochs,
                         double beta_1, double beta_2, int n_steps, int64_t step0, int64_t slot0, float *d_losses,
                         int use_graph, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (!can_fuse(m)) return pyz_fail(PYZ_E_INVALID, "the chained ADAM / VADAM / BSAM runs need a last layer of at most 32 units");
  int rc = check_loss_combo(m);
  if (rc) return rc;
  if ((rc = check_run(m, n_steps, slot0, nullptr)) < 0) return rc;
  if (step0 < 0) return pyz_fail(PYZ_E_INVALID, "negative step count");
  if (!d_theta || !c.m || !c.v || !d_x || !d_y || !d_row_idx || !h_batch_sizes || !h_lr || !d_losses || (!c.bsam && !h_epochs))
    return pyz_fail(PYZ_E_INVALID, "null pointer");
  if (!(beta_1 >= 0.0 && beta_1 < 1.0) || !(beta_2 >= 0.0 && beta_2 < 1.0))
    return pyz_fail(PYZ_E_INVALID, "beta_1 = %g, beta_2 = %g: both must lie in [0, 1)", beta_1, beta_2);
  if (c.perturbs && !(c.c.num_data > 0.0f)) return pyz_fail(PYZ_E_INVALID, "num_data = %g must be positive", (double)c.c.num_data);
  if ((rc = check_run(m, n_steps, slot0, h_batch_sizes, c.bsam ? nullptr : h_epochs)) < 0) return rc;
  if (c.bsam && (rc = need_grad2(m, 1))) return rc;   // grad2 keeps the first pass's gradient
  pyz_mlp_full *f = full(m);
  hipStream_t st = as_stream(stream);
  static const int fuse_perturb = pyz_env_int("PYZ_ADAM_FUSE_PERTURB", 1);
  c.c.perturb = (c.perturbs && fuse_perturb) ? 1 : 0;

  const long long row_stride = m->max_batch;
  const RunBc bc{beta_1, beta_2, h_epochs};
  // each step is launched for its own batch size: the first batch is placed for the forward tiles of the first step
  if ((rc = upload_run_tables(m, h_batch_sizes, h_lr, n_steps, step0, slot0, c.bsam ? nullptr : &bc, d_x, d_row_idx,
                              batch_ahead(m, d_row_idx) ? h_batch_sizes[0] : 0, st)))
    return rc;
  c.c.tab_bc = c.bsam ? nullptr : f->x.tab_bc;
  // fused perturbation: only the first step of the call has nobody in front of it to perturb its weights
  if (c.c.perturb) {
    const unsigned pgrid = (unsigned)cdiv(cdiv(m->D, 4), 256);
    if (c.bsam) PYZ_LAUNCH(k_bsam_perturb, dim3(pgrid), dim3(256), 0, st, d_theta, c.v, m->D, c.bs.inv_n, c.seed, (uint32_t)step0, (const float *)nullptr);
    else PYZ_LAUNCH(k_vadam_perturb, dim3(pgrid), dim3(256), 0, st, d_theta, c.v, m->D, c.c.lam, c.c.num_data, c.seed, (uint32_t)step0, (const float *)nullptr);
  }

  auto step = [&](int s) {
    launch_adam_run_step(m, c, d_theta, d_x, d_y, d_row_idx, h_batch_sizes[s], s & 1, row_stride, d_losses, st);
  };
  int s = 0;
  m->run_graph_steps = m->run_eager_steps = m->run_graph_launches = 0;
  PyzGraphCache<Extra::AR_GRAPHS> &graphs = f->x.adam_graphs;
  graphs.begin_call();
  static const int G = std::min(128, std::max(2, pyz_env_int("PYZ_GRAPH_STEPS", 32) & ~1));   // even: the chunks of a stretch start on one StepCtl slot
  if (use_graph && st != nullptr && !pyz_probe().on) {
    // everything baked into the graphs goes into the key (but the batch sizes: they go into each graph's own signature)
    unsigned long long key = 1469598103934665603ull;
    auto mix = [&](unsigned long long v) { key = (key ^ v) * 1099511628211ull; };
    auto mixf = [&](float v) { unsigned b; memcpy(&b, &v, 4); mix(b); };
    mix(c.bsam ? 0xb5a3ull : 0xada3ull);
    mix((unsigned long long)(uintptr_t)d_theta); mix((unsigned long long)(uintptr_t)c.m); mix((unsigned long long)(uintptr_t)c.v);
    mix((unsigned long long)(uintptr_t)d_x); mix((unsigned long long)(uintptr_t)d_y); mix((unsigned long long)(uintptr_t)d_row_idx);
    mix((unsigned long long)(uintptr_t)d_losses); mix(c.seed); mix((unsigned long long)G);
    mix((unsigned long long)(uintptr_t)m->tab_bs); mix((unsigned long long)(uintptr_t)c.c.tab_bc); mix((unsigned long long)(uintptr_t)m->grad2);
    mix((unsigned long long)c.perturbs); mix((unsigned long long)c.c.perturb); mixf(c.c.lam); mixf(c.c.num_data);
    for (float v : {c.as.b1, c.as.c1, c.as.b2, c.as.c2, c.as.eps, c.as.decay}) mixf(v);
    for (float v : {c.bs.b1, c.bs.c1, c.bs.b2, c.bs.c2, c.bs.lam, c.bs.rho, c.bs.gam, c.bs.inv_n}) mixf(v);
    graphs.rekey(key);
    while (s < n_steps) {
      // a graph holds steps of ONE batch size: chunks of G inside a stretch of equal batches, one graph for the stretch's
      // remainder -- so the ragged batch that ends an epoch is a graph of one step, and a run whose epochs do not line up
      // with its chunks still replays a handful of graphs.  A graph starts on the StepCtl slot it was captured for.
      int stretch = 1;
      while (s + stretch < n_steps && h_batch_sizes[s + stretch] == h_batch_sizes[s]) ++stretch;
      const int len = std::min(G, stretch);
      const unsigned long long sig = ((unsigned long long)h_batch_sizes[s] << 1) | (unsigned long long)(s & 1);
      rc = graphs.launch(len, sig, 0, Extra::AR_GRAPHS, st, [&] {
        for (int k = 0; k < len; ++k) step(s + k);
        return PYZ_OK;
      });
      if (rc) return rc;
      s += len;
      m->run_graph_steps += len;
      ++m->run_graph_launches;
    }
  }
  for (; s < n_steps; ++s) {
    step(s);
    ++m->run_eager_steps;
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_adam_run(pyz_mlp *m, float *d_theta, float *d_m, float *d_v, const float *d_x, const void *d_y,
                 const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr, const int64_t *h_epochs,
                 int n_steps, double beta_1, double beta_2, float denom_eps, float decay, int perturb, float lam, float num_data,
                 int64_t step0, int64_t slot0, uint64_t seed, float *d_losses, int use_graph, void *stream) {
  AdamRunCfg c{};
  c.bsam = false;
  c.m = d_m;
  c.v = d_v;
  c.as = adam_scalars(0.0f, beta_1, beta_2, 1, denom_eps, decay);   // (lr, bc1, bc2: per step, on the device)
  c.c.lam = lam;
  c.c.num_data = num_data;
  c.perturbs = perturb != 0;
  c.seed = seed;
  return adam_run_impl(m, c, d_theta, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, h_epochs, beta_1, beta_2, n_steps, step0, slot0,
                       d_losses, use_graph, stream);
}

int pyz_adam_run_info(const pyz_mlp *m, int32_t *h_captures) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (h_captures) *h_captures = static_cast<const pyz_mlp_full *>(m)->x.adam_graphs.captures;
  return PYZ_OK;
}

int pyz_bsam_run(pyz_mlp *m, float *d_theta, float *d_m, float *d_v, const float *d_x, const void *d_y,
                 const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr, int n_steps, double beta_1,
                 double beta_2, float lam, float rho, float gam, float num_data, int64_t step0, int64_t slot0, uint64_t seed,
                 float *d_losses, int use_graph, void *stream) {
  AdamRunCfg c{};
  c.bsam = true;
  c.m = d_m;
  c.v = d_v;
  // each scalar in float64, rounded to float32 once (see BsamScal)
  c.bs.b1 = (float)beta_1;
  c.bs.c1 = (float)(1.0 - beta_1);
  c.bs.b2 = (float)beta_2;
  c.bs.c2 = (float)(1.0 - beta_2);
  c.bs.lam = lam;
  c.bs.rho = rho;
  c.bs.gam = gam;
  c.bs.inv_n = (float)(1.0 / (double)num_data);
  c.c.num_data = num_data;
  c.perturbs = true;
  c.seed = seed;
  return adam_run_impl(m, c, d_theta, d_x, d_y, d_row_idx, h_batch_sizes, h_lr, nullptr, beta_1, beta_2, n_steps, step0, slot0,
                       d_losses, use_graph, stream);
}

// ---------------------------------------------------------------- H2-H5
int pyz_hmc_step(pyz_mlp *m, float *d_q, int P, const float *d_x, const void *d_y, int n_rows, int L, float epsilon,
                 float mass, float prior_mean, float prior_sigma, const float *d_prior_mean_vec,
                 const float *d_prior_sigma_vec, int burning, const float *h_uniform, int64_t step, uint64_t seed,
                 const float *d_unit_p, float *d_stats, void *stream) {
  int rc = check_call(m, P, n_rows);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_q || !d_x || !d_y || !d_stats || !h_uniform) return pyz_fail(PYZ_E_INVALID, "null pointer");
  if (L < 0) return pyz_fail(PYZ_E_INVALID, "L must be >= 0");
  if ((rc = need_grad(m, P)) || (rc = need_grad2(m, P)) || (rc = need_qsave(m, P))) return rc;   // (also: the gradients of an SVGD phase 1 are gone)
  const int nblk4 = cdiv(cdiv(m->D, 4), 256), nblk1 = cdiv(m->D, 256);
  if ((rc = need_part2(m, (size_t)P * 2 * nblk1 + 8))) return rc;
  hipStream_t st = as_stream(stream);
  pyz_mlp_full *f = full(m);
  float *loss = m->scal;               // [P]
  float *energies = m->scal + m->max_p;  // [P*8]
  float *unif = m->scal + 9 * m->max_p;  // [max_p] uniforms, then one HmcCall
  HmcCall *call_dev = reinterpret_cast<HmcCall *>(m->scal + 10 * m->max_p);  // float index 10 max_p is even
  f->x.hm_path = 0;
  if (!f->x.hm_fed) {   // (inside pyz_hmc_run k_hmc_feed has filled the slot)
    const size_t up_bytes = sizeof(float) * (size_t)m->max_p + sizeof(HmcCall);
    Extra &x = f->x;
    if (!x.up_host) {
      x.up_slot_bytes = (up_bytes + 63) / 64 * 64;
      PYZ_HIP(hipHostMalloc((void **)&x.up_host, x.up_slot_bytes * Extra::UP_SLOTS));
      for (auto &e : x.up_ev) PYZ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const unsigned slot = (unsigned)(x.up_count % Extra::UP_SLOTS);
    if (x.up_count >= (unsigned long long)Extra::UP_SLOTS) PYZ_HIP(hipEventSynchronize(x.up_ev[slot]));  // its last copy has left
    ++x.up_count;
    unsigned char *up = x.up_host + x.up_slot_bytes * slot;
    memcpy(up, h_uniform, sizeof(float) * P);
    HmcCall hc{seed, (uint32_t)step, burning ? 1 : 0};
    memcpy(up + sizeof(float) * (size_t)m->max_p, &hc, sizeof hc);
    PYZ_HIP(hipMemcpyAsync(unif, up, up_bytes, hipMemcpyHostToDevice, st));
    PYZ_HIP(hipEventRecord(x.up_ev[slot], st));
  }
  {
    // small 2-layer models: the whole proposal in one workgroup per chain (pyz_hmc_fused.h)
    const int allow_fused = pyz_env_int("PYZ_HMC_FUSED", 1);  // read per call: tests flip it
    const int I = m->dims[0], H = m->dims[1], C = m->L == 2 ? m->dims[2] : 0;
    const int MIC = (I <= 2 && C <= 2) ? 2 : ((I <= 4 && C <= 4) ? 4 : 8);
    const size_t lds = m->L == 2 ? pyz_hmc_fused_lds_bytes(n_rows, MIC, MIC, C, (int)m->D, m->loss) : 0;
    // (the one-workgroup form needs the whole data set in LDS; the sliced form only its slice)
    const int allow_multi = pyz_env_int("PYZ_HMC_MULTI", 1);  // read per call: tests flip it
    const int rows_per_wg = std::max(16, pyz_env_int("PYZ_HMC_ROWS_PER_WG", 96));
    const int NW = std::min(PYZ_HM_MAXW, n_rows / rows_per_wg);
    const size_t mlds = m->L == 2 ? pyz_hmc_multi_lds_bytes(cdiv(n_rows, std::max(NW, 1)) + 1, MIC, MIC, C, (int)m->D, m->loss) : 0;
    const bool multi_ok = allow_multi && NW >= 2 && P <= pyz_env_int("PYZ_HMC_MULTI_MAX_CHAINS", 16) && mlds <= 150 * 1024;
    if (allow_fused && !d_prior_mean_vec && !d_prior_sigma_vec && m->L == 2 && I <= PYZ_HF_MAXI && C <= PYZ_HF_MAXC && H + C <= 64 &&
        (lds <= 150 * 1024 || multi_ok) && m->acts[0] != PYZ_ACT_SOFTMAX) {
      HmcFusedArgs f{};
      f.q = d_q;
      f.x = d_x;
      f.y = d_y;
      f.N = n_rows;
      f.I = I;
      f.H = H;
      f.C = C;
      f.D = (int)m->D;
      f.act_hidden = m->acts[0];
      f.act_last = m->acts[1];
      f.loss = m->loss;
      f.L = L;
      f.epsilon = epsilon;
      f.m = mass;
      f.prior_mean = prior_mean;
      f.prior_sigma = prior_sigma;
      f.burning = burning;
      f.uniform = unif;
      f.seed = seed;
      f.step = (uint32_t)step;
      f.unit_p = d_unit_p;
      f.stats = d_stats;
      void (*kern)(HmcFusedArgs) = nullptr;
      const int bucket = (I <= 2 && C <= 2) ? 0 : ((I <= 4 && C <= 4) ? 1 : 2);
#define PYZ_HF_PICK(ACT)                                                                         \
  kern = bucket == 0 ? k_hmc_fused<2, 2, ACT> : (bucket == 1 ? k_hmc_fused<4, 4, ACT> : k_hmc_fused<8, 8, ACT>)
      switch (m->acts[0]) {
        case PYZ_ACT_RELU: PYZ_HF_PICK(PYZ_ACT_RELU); break;
        case PYZ_ACT_TANH: PYZ_HF_PICK(PYZ_ACT_TANH); break;
        case PYZ_ACT_SIGMOID: PYZ_HF_PICK(PYZ_ACT_SIGMOID); break;
        default: PYZ_HF_PICK(PYZ_ACT_LINEAR); break;
      }
#undef PYZ_HF_PICK
      // few chains: spread each one over NW workgroups, one launch per gradient evaluation (pyz_hmc_multi.h);
      // many chains: one workgroup per chain, the whole proposal in one launch
      if (multi_ok) {
        HmcMultiArgs mm{};
        mm.f = f;
        mm.NW = NW;
        mm.max_rows = cdiv(n_rows, NW) + 1;
        const size_t D = (size_t)m->D;
        const size_t n_state = 2 * (size_t)P * D, n_slab = 2 * (size_t)P * NW * D;
        const size_t bytes = sizeof(float) * (2 * n_state + n_slab + 4 * (size_t)P) + sizeof(double) * 2 * (size_t)P * NW + 64;
        pyz_mlp_full *fm = full(m);
        if ((rc = ensure_bytes(&fm->x.hm_buf, &fm->x.hm_cap, bytes, m))) return rc;
        mm.lpart = reinterpret_cast<double *>(fm->x.hm_buf);  // doubles first: 8-byte aligned
        mm.qw = reinterpret_cast<float *>(mm.lpart + 2 * (size_t)P * NW);
        mm.pw = mm.qw + n_state;
        mm.slab = mm.pw + n_state;
        mm.scal = mm.slab + n_slab;
        void (*kmulti)(HmcMultiArgs) = nullptr;
#define PYZ_HM_PICK(ACT)                                                                         \
  kmulti = bucket == 0 ? k_hmc_multi<2, 2, ACT> : (bucket == 1 ? k_hmc_multi<4, 4, ACT> : k_hmc_multi<8, 8, ACT>)
        switch (m->acts[0]) {
          case PYZ_ACT_RELU: PYZ_HM_PICK(PYZ_ACT_RELU); break;
          case PYZ_ACT_TANH: PYZ_HM_PICK(PYZ_ACT_TANH); break;
          case PYZ_ACT_SIGMOID: PYZ_HM_PICK(PYZ_ACT_SIGMOID); break;
          default: PYZ_HM_PICK(PYZ_ACT_LINEAR); break;
        }
#undef PYZ_HM_PICK
        if (mlds > 64 * 1024)
          PYZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kmulti), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds));
        mm.call = call_dev;
        // the whole proposal as one resident launch (k_hmc_resident) when its NW x chains workgroups fit the chip at once
        void (*kres)(HmcMultiArgs) = nullptr;
#define PYZ_HR_PICK(ACT)                                                                         \
  kres = bucket == 0 ? k_hmc_resident<2, 2, ACT> : (bucket == 1 ? k_hmc_resident<4, 4, ACT> : k_hmc_resident<8, 8, ACT>)
        switch (m->acts[0]) {
          case PYZ_ACT_RELU: PYZ_HR_PICK(PYZ_ACT_RELU); break;
          case PYZ_ACT_TANH: PYZ_HR_PICK(PYZ_ACT_TANH); break;
          case PYZ_ACT_SIGMOID: PYZ_HR_PICK(PYZ_ACT_SIGMOID); break;
          default: PYZ_HR_PICK(PYZ_ACT_LINEAR); break;
        }
#undef PYZ_HR_PICK
        bool resident = pyz_env_int("PYZ_HMC_RESIDENT", 1) != 0 && NW * P <= pyz_cu_count();   // (read per call: tests flip it)
        if (resident) {
          if (mlds > 64 * 1024)
            PYZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kres), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds));
          int per_cu = 0;
          if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(kres), PYZ_HM_THREADS, mlds) != hipSuccess || per_cu < 1)
            resident = false;
        }
        if (resident) {
          const int Dp = (int)((D + 2 + 31) / 32 * 32);
          const size_t rbytes = 256 + sizeof(unsigned long long) * 2 * (size_t)P * NW * Dp;
          const size_t had = fm->x.hm_res_cap;
          if ((rc = ensure_bytes(&fm->x.hm_res_buf, &fm->x.hm_res_cap, rbytes, m))) return rc;
          if (fm->x.hm_res_cap != had)   // a fresh buffer: epochs and tags start at zero (the kernel's tags are >= 1 and only grow)
            PYZ_HIP(hipMemsetAsync(fm->x.hm_res_buf, 0, fm->x.hm_res_cap, st));
          mm.epoch = reinterpret_cast<unsigned *>(fm->x.hm_res_buf);
          mm.gran = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(fm->x.hm_res_buf) + 256);
          mm.Dp = Dp;
          mm.spin_limit = pyz_env_int("PYZ_HMC_SPIN_LIMIT", 1 << 20);
#ifdef PYZ_HMC_DIAG
          mm.diag = pyz_env_int("PYZ_HMC_DIAG", 0);
#endif
        }
        // one graph per (kernel, shapes, pointers, scalars): a proposal is L + 2 dependent launches (resident: a memset and one launch)
        unsigned long long key = 1469598103934665603ull;
        auto mix = [&](unsigned long long v) { key = (key ^ v) * 1099511628211ull; };
        mix((unsigned long long)(uintptr_t)(resident ? kres : kmulti)); mix((unsigned long long)(uintptr_t)mm.gran); mix((unsigned long long)mm.spin_limit + 7 * (unsigned long long)mm.diag); mix((unsigned long long)L); mix((unsigned long long)P); mix((unsigned long long)NW);
        mix((unsigned long long)n_rows); mix((unsigned long long)(uintptr_t)d_q); mix((unsigned long long)(uintptr_t)d_x);
        mix((unsigned long long)(uintptr_t)d_y); mix((unsigned long long)(uintptr_t)d_unit_p); mix((unsigned long long)(uintptr_t)d_stats);
        mix((unsigned long long)(uintptr_t)fm->x.hm_buf); mix((unsigned long long)(uintptr_t)st);
        unsigned fbits[4];
        memcpy(&fbits[0], &epsilon, 4); memcpy(&fbits[1], &mass, 4); memcpy(&fbits[2], &prior_mean, 4); memcpy(&fbits[3], &prior_sigma, 4);
        for (unsigned b : fbits) mix(b);
        const int use_graph = fm->x.hm_fed ? 0 : pyz_env_int("PYZ_HMC_GRAPH", 1);   // (read per call: tests flip it; a run captures graphs of its own)
        fm->x.hm_path = resident ? 3 : 2;
        fm->x.hm_sig = key;
        auto launch_all = [&]() {
          if (resident) {
            PYZ_LAUNCH(kres, dim3(NW, P), dim3(PYZ_HM_THREADS), mlds, st, mm);
            return;
          }
          for (int t = 0; t <= L; ++t) {
            mm.t = t;
            PYZ_LAUNCH(kmulti, dim3(NW, P), dim3(PYZ_HM_THREADS), mlds, st, mm);
          }
          PYZ_LAUNCH(k_hmc_multi_final, dim3(P), dim3(PYZ_HM_THREADS), 0, st, mm);
        };
        if (!use_graph || st == nullptr) {  // the legacy default stream cannot be captured
          launch_all();
          PYZ_LAUNCH_CHECK();
          return PYZ_OK;
        }
        fm->x.hm_graphs.rekey(key);
        return fm->x.hm_graphs.launch(1, 0, 0, 1, st, [&] {
          launch_all();
          return PYZ_OK;
        });
      }
      if (lds > 64 * 1024)
        PYZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      PYZ_LAUNCH(kern, dim3(P), dim3(PYZ_HF_THREADS), lds, st, f);
      full(m)->x.hm_path = 1;
      PYZ_LAUNCH_CHECK();
      return PYZ_OK;
    }
  }
  if ((rc = set_ctl(m, 0, n_rows, 0.0f, step, 0, 0, st))) return rc;
  HmcArgs a{};
  a.q = d_q;
  a.p = m->grad2;
  a.qsave = m->qsave;
  a.grad = m->grad;
  a.D = m->D;
  a.m = mass;
  a.prior_mean = prior_mean;
  a.prior_sigma = prior_sigma;
  a.pm_vec = d_prior_mean_vec;
  a.ps_vec = d_prior_sigma_vec;
  a.n_train = (float)n_rows;
  a.seed = seed;
  a.step = (uint32_t)step;
  a.unit_p = d_unit_p;
  a.part = f->x.part2;
  auto grad_eval = [&]() {
    WgradArgs u{};
    u.mode = PYZ_UPD_NONE;
    u.grad = m->grad;
    u.grad_pstride = m->D;
    launch_loss_backward(m, d_q, m->D, P, d_x, d_y, nullptr, n_rows, m->ctl, true, u, st);
    PYZ_LAUNCH(k_loss_finalize, dim3(P), dim3(64), 0, st, m->part, m->cur_nblk, m->ctl, loss, m->nonfinite);
  };
  // momentum, snapshot, K0 and the prior part of U0
  a.nblk = nblk4;
  PYZ_LAUNCH(k_hmc_begin, dim3(nblk4, P), dim3(256), 0, st, a);
  grad_eval();
  PYZ_LAUNCH(k_hmc_energy_finalize, dim3(P), dim3(64), 0, st, f->x.part2, nblk4, loss, a.n_train, mass, energies, 0);
  // half kick + first drift (HMC.py:82-84); with L == 0 the two half kicks share the gradient
  a.nblk = nblk1;
  if (L == 0) {
    a.kick1 = epsilon / 2;
    a.kick2 = epsilon / 2;
    a.drift = 0.0f;
    PYZ_LAUNCH(k_hmc_kick_drift, dim3(nblk1, P), dim3(256), 0, st, a);
  } else {
    a.kick1 = epsilon / 2;
    a.kick2 = 0.0f;
    a.drift = epsilon / mass;
    PYZ_LAUNCH(k_hmc_kick_drift, dim3(nblk1, P), dim3(256), 0, st, a);
    for (int i = 1; i <= L; ++i) {
      grad_eval();
      a.kick1 = epsilon;
      if (i < L) {
        a.kick2 = 0.0f;
        a.drift = epsilon / mass;
      } else {  // last full kick and the closing half kick use the same gradient (HMC.py:86-87)
        a.kick2 = epsilon / 2;
        a.drift = 0.0f;
      }
      PYZ_LAUNCH(k_hmc_kick_drift, dim3(nblk1, P), dim3(256), 0, st, a);
    }
  }
  // K1, U1 (the loss of the last gradient evaluation is the loss at the proposal)
  PYZ_LAUNCH(k_hmc_end_energy, dim3(nblk1, P), dim3(256), 0, st, a);
  PYZ_LAUNCH(k_hmc_energy_finalize, dim3(P), dim3(64), 0, st, f->x.part2, nblk1, loss, a.n_train, mass, energies, 1);
  PYZ_LAUNCH(k_hmc_accept, dim3(cdiv(P, 64)), dim3(64), 0, st, energies, unif, burning, d_stats, P);
  PYZ_LAUNCH(k_hmc_restore, dim3(nblk1, P), dim3(256), 0, st, d_q, m->qsave, d_stats, m->D);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// The quiet HMC.train (HMC.py:106-125 around HMC.py:74-104) as one device-resident run: n_steps proposals of
// pyz_hmc_step, each between k_hmc_feed (its uniforms and HmcCall out of the run's table) and k_hmc_record (its
// statistics to their slot, the sample record), with no host work in between.  The proposal itself is launched by
// pyz_hmc_step's own dispatch (Extra::hm_fed: no upload, no graph of its own).  The sliced forms (k_hmc_multi,
// k_hmc_resident) read their scalars from the device: their proposals are captured, feed and record included, into
// graphs of PYZ_HMC_RUN_CHUNK proposals and one of the exact remaining length, kept as sgld_run_impl keeps its graphs.
// k_hmc_fused and the generic sequence take the step and the burning flag as kernel arguments: they are launched
// eagerly from the loop below (the host knows both; the uniforms still come from the device), without a
// synchronisation.  The first proposal of a call is always eager: it sizes the buffers the dispatch grows lazily
// (nothing is allocated or cleared inside a capture) and tells which form the shape takes.
// Extra::hm_fed is state of the plan: like every entry point that uses the plan's workspace, a plan is driven by one host
// thread at a time (include/pyz.h), and pyz_hmc_step is not called on it from elsewhere while this function runs.
int pyz_hmc_run(pyz_mlp *m, float *d_q, int P, const float *d_x, const void *d_y, int n_rows, int L, float epsilon,
                float mass, float prior_mean, float prior_sigma, const float *d_prior_mean_vec,
                const float *d_prior_sigma_vec, const float *h_uniform, int n_steps, int n_burn, int64_t step0,
                int64_t slot0, uint64_t seed, float *d_stats_all, float *d_samples, int32_t *d_freq, int32_t *d_count,
                int cap, int32_t *d_fail, int use_graph, void *stream) {
  // argument errors first: none of them touches the plan or the GPU
  if (!m || !d_q || !d_x || !d_y || !h_uniform || !d_stats_all || !d_samples || !d_freq || !d_count || !d_fail)
    return pyz_fail(PYZ_E_INVALID, "pyz_hmc_run: null pointer");
  if (n_steps <= 0) return pyz_fail(PYZ_E_INVALID, "pyz_hmc_run: n_steps must be positive");
  if (n_burn < 0 || n_burn > n_steps) return pyz_fail(PYZ_E_INVALID, "pyz_hmc_run: n_burn %d outside [0, %d]", n_burn, n_steps);
  if (cap < 1) return pyz_fail(PYZ_E_INVALID, "pyz_hmc_run: cap must be at least 1 (the starting q is a row)");
  if (step0 < 0) return pyz_fail(PYZ_E_INVALID, "pyz_hmc_run: negative step0");
  if (slot0 < 0 || slot0 + n_steps > 0x7fffffff) return pyz_fail(PYZ_E_INVALID, "pyz_hmc_run: slot0 out of range");
  int rc = check_call(m, P, n_rows);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (L < 0) return pyz_fail(PYZ_E_INVALID, "L must be >= 0");
  if (m->D > 0x7fffffff / 2) return pyz_fail(PYZ_E_SHAPE, "pyz_hmc_run: the model is too large for the sample record's indexing");
  hipStream_t st = as_stream(stream);
  pyz_mlp_full *f = full(m);
  Extra &x = f->x;
  // ---- the run's device words and the uniform table
  const size_t snap_off = 256, stats_off = snap_off + (sizeof(int32_t) * (size_t)m->max_p + 63) / 64 * 64;
  if (!x.hr_buf) {
    size_t have = 0;
    if ((rc = ensure_bytes(&x.hr_buf, &have, stats_off + sizeof(float) * 8 * (size_t)m->max_p, m))) return rc;
  }
  static_assert(sizeof(HmcRunCtl) <= 256, "HmcRunCtl outgrew its slot");
  HmcRunArgs ra{};
  ra.ctl = reinterpret_cast<HmcRunCtl *>(x.hr_buf);
  ra.snap_count = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(x.hr_buf) + snap_off);
  float *run_stats = reinterpret_cast<float *>(static_cast<unsigned char *>(x.hr_buf) + stats_off);
  ra.unif = m->scal + 9 * m->max_p;                                   // the slot pyz_hmc_step uploads to
  ra.call = reinterpret_cast<HmcCall *>(m->scal + 10 * m->max_p);
  ra.q = d_q;
  ra.stats = run_stats;
  ra.nonfinite = m->nonfinite;
  ra.P = P;
  ra.D = (int)m->D;
  const size_t n_tab = (size_t)n_steps * P;
  if (x.hr_tab_cap < n_tab) {   // (the table's address is a word of HmcRunCtl, not baked into the graphs)
    if (x.hr_tab) {
      PYZ_HIP(hipDeviceSynchronize());   // (rare: an earlier run on another stream may still read it)
      PYZ_HIP(hipFree(x.hr_tab));
      x.hr_tab = nullptr;
      x.hr_tab_cap = 0;
    }
    const size_t cap_f = std::max<size_t>(n_tab, 16384);
    PYZ_HIP(hipMalloc((void **)&x.hr_tab, sizeof(float) * cap_f));
    m->ws_bytes += sizeof(float) * cap_f;
    x.hr_tab_cap = cap_f;
  }
  if (x.hr_host_cap < sizeof(float) * n_tab) {
    if (x.hr_host) {
      PYZ_HIP(hipDeviceSynchronize());
      PYZ_HIP(hipHostFree(x.hr_host));
      x.hr_host = nullptr;
    } else {
      for (auto &e : x.hr_ev) PYZ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const size_t cap_b = std::max<size_t>(sizeof(float) * n_tab, 65536);
    PYZ_HIP(hipHostMalloc((void **)&x.hr_host, 2 * cap_b));
    x.hr_host_cap = cap_b;
    x.hr_count = 0;
  }
  {
    const unsigned slot = (unsigned)(x.hr_count & 1);
    if (x.hr_count >= 2) PYZ_HIP(hipEventSynchronize(x.hr_ev[slot]));   // the copy of the run before the previous one has left
    ++x.hr_count;
    unsigned char *hb = x.hr_host + slot * x.hr_host_cap;
    std::memcpy(hb, h_uniform, sizeof(float) * n_tab);
    PYZ_HIP(hipMemcpyAsync(x.hr_tab, hb, sizeof(float) * n_tab, hipMemcpyHostToDevice, st));
    PYZ_HIP(hipEventRecord(x.hr_ev[slot], st));
  }
  HmcRunCtl init{};
  init.unif_tab = x.hr_tab;
  init.stats_all = d_stats_all;
  init.samples = d_samples;
  init.freq = d_freq;
  init.count = d_count;
  init.fail = d_fail;
  init.seed = seed;
  init.step0 = step0;
  init.slot0 = slot0;
  init.n_burn = n_burn;
  init.cap = cap;
  PYZ_LAUNCH(k_hmc_run_begin, dim3(1), dim3(1), 0, st, ra.ctl, init);

  const dim3 rgrid(cdiv(cdiv(m->D, 4), 256), P);
  struct Fed {   // pyz_hmc_step below takes its scalars from the device; whatever way this call ends, the next one uploads again
    bool &on;
    explicit Fed(bool &b) : on(b) { on = true; }
    ~Fed() { on = false; }
  } fed(x.hm_fed);
  auto proposal = [&](int i) -> int {
    PYZ_LAUNCH(k_hmc_feed, rgrid, dim3(256), 0, st, ra);
    const int prc = pyz_hmc_step(m, d_q, P, d_x, d_y, n_rows, L, epsilon, mass, prior_mean, prior_sigma, d_prior_mean_vec,
                                 d_prior_sigma_vec, i < n_burn ? 1 : 0, h_uniform, step0 + i, seed, nullptr, run_stats, stream);
    if (prc) return prc;
    PYZ_LAUNCH(k_hmc_record, rgrid, dim3(256), 0, st, ra);
    return PYZ_OK;
  };
  m->run_graph_steps = m->run_eager_steps = m->run_graph_launches = 0;
  x.hmc_run_graphs.begin_call();
  int s = 0;
  if ((rc = proposal(s))) return rc;
  ++s;
  ++m->run_eager_steps;
  const int G = std::min(256, std::max(1, pyz_env_int("PYZ_HMC_RUN_CHUNK", 16)));   // (read per call, mixed into the key)
  if (use_graph && st != nullptr && !pyz_probe().on && x.hm_path >= 2) {
    // everything baked into the graphs goes into the key: what the sliced launches bake in (hm_sig: kernel, shapes,
    // pointers, scalars, stream) and the arguments of the feed / record launches
    unsigned long long key = x.hm_sig;
    auto mix = [&](unsigned long long v) { key = (key ^ v) * 1099511628211ull; };
    mix((unsigned long long)(uintptr_t)x.hr_buf); mix((unsigned long long)(uintptr_t)ra.unif); mix((unsigned long long)m->max_p);
    mix((unsigned long long)m->D); mix((unsigned long long)G);
    x.hmc_run_graphs.rekey(key);
    while (s < n_steps) {
      const int len = std::min(G, n_steps - s);
      const bool rest = len < G;   // the remainder: its own graph, by exact length in slots 1 ..; slot 0 holds the full chunk
      rc = x.hmc_run_graphs.launch(len, 0, rest ? 1 : 0, rest ? PYZ_GRAPH_CHUNKS : 1, st, [&] {
        int crc = PYZ_OK;
        for (int k = 0; k < len && !crc; ++k) crc = proposal(s + k);   // (step and burning ride in HmcCall: the graph fits any position)
        return crc;
      });
      if (rc) return rc;
      s += len;
      m->run_graph_steps += len;
      ++m->run_graph_launches;
    }
  }
  for (; s < n_steps; ++s) {
    if ((rc = proposal(s))) return rc;
    ++m->run_eager_steps;
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_hmc_run_info(const pyz_mlp *m, int32_t *h_captures) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (h_captures) *h_captures = static_cast<const pyz_mlp_full *>(m)->x.hmc_run_graphs.captures;
  return PYZ_OK;
}

// one-time check of the lane layout k_svgd_gram_tile assumes for v_mfma_f64_16x16x4_f64
static bool mfma_f64_layout_ok(hipStream_t st) {
  static int state = -1;  // -1 unknown, 0 no, 1 yes
  if (state >= 0) return state == 1;
  int *d = nullptr;
  int h[512];
  state = 0;
  if (hipMalloc((void **)&d, sizeof h) != hipSuccess) return false;
  PYZ_LAUNCH(k_probe_mfma_f64, dim3(1), dim3(64), 0, st, d);
  if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
    bool ok = true;
    for (int l = 0; l < 64 && ok; ++l)
      for (int r = 0; r < 4; ++r)
        if (h[4 * l + r] != (l >> 4) + 4 * r || h[256 + 4 * l + r] != (l & 15)) ok = false;
    state = ok ? 1 : 0;
  }
  (void)hipFree(d);
  return state == 1;
}

// ---------------------------------------------------------------- V2-V4
// phase 1 of SVGD.step: all loss gradients of the local particles in one particle-batched pass -- g_i depends on
// particle i only (SVGD.py:104-111); they stay in the plan's gradient buffer, the losses in its scalars
static int svgd_gradients_impl(pyz_mlp *m, const float *d_particles, int n_local, const float *d_x, const void *d_y,
                               const int32_t *d_row_idx, int batch, hipStream_t st) {
  int rc = check_call(m, n_local, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_particles || !d_x || !d_y) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if ((rc = need_grad(m, n_local))) return rc;
  m->grad_owner = 1;
  m->grad_rows = n_local;
  set_ctl_lazy(m, batch, 0.0f, 0);   // the first kernel of the pass carries the step scalars
  WgradArgs u{};
  u.mode = PYZ_UPD_NONE;
  u.grad = m->grad;
  u.grad_pstride = m->D;
  const bool fused = can_fuse(m);
  if (fused) u.ploss = m->scal;      // per-particle losses in the weight-gradient launch (every particle's spare workgroup)
  launch_loss_backward(m, d_particles, m->D, n_local, d_x, d_y, d_row_idx, batch, m->ctl, true, u, st);
  if (!fused) PYZ_LAUNCH(k_loss_finalize, dim3(n_local), dim3(64), 0, st, m->part, m->cur_nblk, m->ctl, m->scal, m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---- phase 2 on a snapshot, all rows at once (Jacobi; M <= 64, local rows in multiples of four), in two halves:
//   kernel matrix   the squared distances of the local rows against the snapshot (Gram matrix on the float64 matrix
//                   cores, or pairwise), [the median-heuristic bandwidth,] K rows and their sums -- a function of the
//                   snapshot ALONE: it may run on a second stream while phase 1 computes the gradients;
//   combine         phi, the legacy Adam step and the step's loss for every local row -- needs both.
// Both carve the same layout out of the plan's float64 scratch.
struct TileLayout {
  SvgdTileArgs ta;   // the local rows
  SvgdTileArgs td;   // the distance pass (all rows under the median heuristic)
};

static bool svgd_tile_shape(int n_local, int n_total, int row0, const float *d_all, const float *d_particles) {
  return n_total <= 64 && row0 % 4 == 0 && n_local % 4 == 0 && d_all != d_particles;
}

static int svgd_tile_layout(pyz_mlp *m, const float *d_all, int n_total, int row0, int n_local, float gamma, TileLayout &L) {
  const bool median = gamma == PYZ_SVGD_GAMMA_MEDIAN;
  SvgdTileArgs ta{};
  ta.all = d_all;
  ta.D = m->D;
  ta.M = n_total;
  ta.n_local = n_local;
  ta.row0 = row0;
  ta.gamma = gamma;
  ta.range = PYZ_SV_E * cdiv(m->D, 256LL * PYZ_SV_E);  // one round of workgroups on the 256 CUs
  ta.nblk = cdiv(m->D, ta.range);
  // the median heuristic (SVGD.py:165-181) needs the squared distances of ALL pairs: the distance pass then covers
  // every row of the gathered matrix on every rank (the matrix is read once either way)
  const int dist_rows = median ? n_total : n_local, dist_row0 = median ? 0 : row0;
  const size_t n_part = (size_t)dist_rows * ta.nblk * 64, n_k = (size_t)n_local * 64, n_diag = (size_t)ta.nblk * 64;
  const size_t n_dmat = median ? (size_t)n_total * 64 + 8 : 0;
  const int rc = need_part2(m, n_part + n_k + 2 * (size_t)n_local + n_diag + n_dmat + 16, /*keep_kernel_matrix=*/true);
  if (rc) return rc;
  ta.part = full(m)->x.part2;
  ta.kmat = ta.part + n_part;
  ta.ksumd = ta.kmat + n_k;
  ta.ksum = reinterpret_cast<float *>(ta.ksumd + n_local);
  double *after_ksum = ta.ksumd + n_local + (n_local + 1) / 2 + 1;
  SvgdTileArgs td = ta;
  td.n_local = dist_rows;
  td.row0 = dist_row0;
  td.diag = after_ksum;                        // (only read when the Gram form ran: see the kernel-matrix half)
  if (median) {
    td.dmat = after_ksum + n_diag;             // (M, 64) squared distances, then the bandwidth
    td.gamma_dev = td.dmat + (size_t)n_total * 64;
    ta.dmat = td.dmat;
    ta.gamma_dev = td.gamma_dev;
  }
  L.ta = ta;
  L.td = td;
  return PYZ_OK;
}

static int svgd_check_rows(const pyz_mlp *m, int n_local, int n_total, int row0, float gamma) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (n_local <= 0 || n_local > m->max_p) return pyz_fail(PYZ_E_SHAPE, "particle count %d outside [1, %d] of the plan", n_local, m->max_p);
  if (n_total < n_local || row0 < 0 || row0 + n_local > n_total) return pyz_fail(PYZ_E_INVALID, "rows [%d, %d) outside the %d particles", row0, row0 + n_local, n_total);
  if (n_total > 1024) return pyz_fail(PYZ_E_INVALID, "more than 1024 particles");
  if (gamma != PYZ_SVGD_GAMMA_MEDIAN && !(gamma > 0.0f)) return pyz_fail(PYZ_E_INVALID, "gamma must be positive (or PYZ_SVGD_GAMMA_MEDIAN)");
  return PYZ_OK;
}

// the distance pass over blocks [blk0, blk0 + n_blocks) of the layout (partials of td's rows into the plan's scratch)
static void svgd_launch_distance_pass(SvgdTileArgs td, int blk0, int n_blocks, bool gram, hipStream_t st) {
  td.blk0 = blk0;
  if (gram) {
    // a shard whose rows lie in one or two row blocks of 16 computes those blocks only; every other row range takes the
    // 10 upper blocks of the whole matrix (identical bits per entry, pyz_kernels.h)
    const int rb_lo = td.row0 >> 4, rb_hi = (td.row0 + td.n_local - 1) >> 4;
    const size_t gr_lds = pyz_svgd_gram_lds_bytes();
    if (rb_hi == rb_lo) PYZ_LAUNCH((k_svgd_gram_tile<1, false>), dim3(n_blocks), dim3(512), gr_lds, st, td);
    else if (rb_hi == rb_lo + 1) PYZ_LAUNCH((k_svgd_gram_tile<2, false>), dim3(n_blocks), dim3(512), gr_lds, st, td);
    else PYZ_LAUNCH((k_svgd_gram_tile<4, true>), dim3(n_blocks), dim3(512), gr_lds, st, td);
  } else {
    PYZ_LAUNCH(k_svgd_dist_tile, dim3(n_blocks), dim3(256), 0, st, td);
  }
}

// d_groups != nullptr: the group sums of the partial squared distances of ALL rows, gathered from the ranks that each
// summed some groups (pyz_svgd_gram_groups); nullptr: this device runs the whole distance pass itself
static int svgd_kernel_matrix_impl(pyz_mlp *m, const float *d_all, int n_total, int row0, int n_local, float gamma,
                                   const double *d_groups, hipStream_t st) {
  int rc = svgd_check_rows(m, n_local, n_total, row0, gamma);
  if (rc) return rc;
  if (!d_all) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  const bool median = gamma == PYZ_SVGD_GAMMA_MEDIAN;
  if (!svgd_tile_shape(n_local, n_total, row0, d_all, nullptr) || (median && n_total % 4 != 0))
    return pyz_fail(PYZ_E_INVALID, "the kernel matrix of a snapshot needs at most 64 particles and local rows [row0, row0 + n) in "
                                   "multiples of four (the median heuristic: the particle count too)");
  m->km_valid = false;
  TileLayout L;
  if ((rc = svgd_tile_layout(m, d_all, n_total, row0, n_local, gamma, L))) return rc;
  L.ta.groups = L.td.groups = d_groups;
  if (!d_groups) {
    // distances through the Gram matrix on the float64 matrix cores when the instruction's lane layout is the
    // one the kernel assumes (probed once); else the pairwise float64 VALU kernel
    const int gram_on = pyz_env_int("PYZ_SVGD_GRAM", 1);  // read per call: tests flip it
    svgd_launch_distance_pass(L.td, 0, L.td.nblk, gram_on && mfma_f64_layout_ok(st), st);
  }
  if (median) {
    PYZ_LAUNCH(k_svgd_kmat, dim3(n_total), dim3(1024), 0, st, L.td, 1);   // distances only
    PYZ_LAUNCH(k_svgd_median, dim3(1), dim3(1024), 0, st, L.td);
  }
  PYZ_LAUNCH(k_svgd_kmat, dim3(n_local), dim3(1024), 0, st, L.ta, 0);
  PYZ_LAUNCH_CHECK();
  m->km_valid = true;
  m->km_all = d_all;
  m->km_total = n_total;
  m->km_row0 = row0;
  m->km_local = n_local;
  m->km_gamma = gamma;
  return PYZ_OK;
}

// the distance pass of groups [g_lo, g_hi) of the PYZ_SVGD_GROUPS groups of blocks (this rank's share of the ELEMENTS),
// all rows; the group sums go to the caller's (PYZ_SVGD_GROUPS, 64, 64) buffer at the groups' places
static int svgd_gram_groups_impl(pyz_mlp *m, const float *d_all, int n_total, int g_lo, int g_hi, double *d_groups, hipStream_t st) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (!d_all || !d_groups) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n_total < 4 || n_total > 64 || n_total % 4 != 0) return pyz_fail(PYZ_E_INVALID, "the grouped distance pass takes 4 .. 64 particles in multiples of four");
  if (g_lo < 0 || g_hi > PYZ_SVGD_GROUPS || g_lo >= g_hi) return pyz_fail(PYZ_E_INVALID, "groups [%d, %d) outside [0, %d)", g_lo, g_hi, PYZ_SVGD_GROUPS);
  m->km_valid = false;
  TileLayout L;
  // (the layout of the WHOLE matrix: partials of all rows; gamma does not enter the distance pass)
  int rc = svgd_tile_layout(m, d_all, n_total, 0, n_total, 1.0f, L);
  if (rc) return rc;
  const int nblk = L.td.nblk, nb8 = cdiv(nblk, PYZ_SVGD_GROUPS);
  const int blk0 = std::min(g_lo * nb8, nblk), blk1 = std::min(g_hi * nb8, nblk);
  const int gram_on = pyz_env_int("PYZ_SVGD_GRAM", 1);
  if (blk1 > blk0) svgd_launch_distance_pass(L.td, blk0, blk1 - blk0, gram_on && mfma_f64_layout_ok(st), st);
  PYZ_LAUNCH(k_svgd_group_reduce, dim3(n_total, g_hi - g_lo), dim3(128), 0, st, (const double *)L.td.part, nblk, g_lo, d_groups);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// The Jacobi sweep reads every row of the snapshot while other workgroups of the same launch write d_particles: rows
// written inside [d_all, d_all + M D) would be read half old, half new (neither sweep, not reproducible)
static int svgd_check_snapshot(const pyz_mlp *m, const float *d_particles, int n_local, const float *d_all, int n_total, int sweep) {
  if (sweep != PYZ_SWEEP_JACOBI || !m || !d_particles || !d_all) return PYZ_OK;
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(d_particles), a0 = reinterpret_cast<uintptr_t>(d_all);
  const uintptr_t row = sizeof(float) * (uintptr_t)m->D;
  if (p0 < a0 + (uintptr_t)n_total * row && a0 < p0 + (uintptr_t)n_local * row)
    return pyz_fail(PYZ_E_INVALID, "the Jacobi sweep needs a snapshot separate from the rows it writes (d_particles overlaps d_all)");
  return PYZ_OK;
}

static int svgd_check_gradients(const pyz_mlp *m, int n_local) {
  if (!m->grad || m->grad_owner != 1 || m->grad_rows != n_local)
    return pyz_fail(PYZ_E_INVALID, "no gradients of these %d particles in the plan: pyz_svgd_gradients must be the last "
                                   "gradient-producing call on it", n_local);
  return PYZ_OK;
}

static int svgd_combine_impl(pyz_mlp *m, float *d_particles, int n_local, const float *d_all, int n_total, int row0,
                             float *d_adam_m, float *d_adam_v, float lr, float gamma, int64_t t, float *d_loss, hipStream_t st) {
  int rc = svgd_check_rows(m, n_local, n_total, row0, gamma);
  if (rc) return rc;
  if (!d_particles || !d_all || !d_adam_m || !d_adam_v || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (t < 1) return pyz_fail(PYZ_E_INVALID, "Adam step t must be >= 1");
  if ((rc = svgd_check_snapshot(m, d_particles, n_local, d_all, n_total, PYZ_SWEEP_JACOBI))) return rc;
  if ((rc = svgd_check_gradients(m, n_local))) return rc;
  if (!m->km_valid || m->km_all != d_all || m->km_total != n_total || m->km_row0 != row0 || m->km_local != n_local || m->km_gamma != gamma)
    return pyz_fail(PYZ_E_INVALID, "pyz_svgd_combine without the kernel matrix of this snapshot (pyz_svgd_kernel_matrix with the "
                                   "same d_all, rows and gamma must precede it, with no other call on the plan's scratch in between)");
  TileLayout L;
  if ((rc = svgd_tile_layout(m, d_all, n_total, row0, n_local, gamma, L))) return rc;
  SvgdTileArgs &ta = L.ta;
  ta.particles = d_particles;
  ta.adam_m = d_adam_m;
  ta.adam_v = d_adam_v;
  ta.grad = m->grad;
  const double b1t = std::pow(0.9, (double)t), b2t = std::pow(0.999, (double)t);
  ta.lr_t = (float)((double)lr * std::sqrt(1.0 - b2t) / (1.0 - b1t));
  ta.loss_in = m->scal;   // [n_local], written by phase 1
  ta.loss_out = d_loss;
  PYZ_LAUNCH(k_svgd_update_tile, dim3(cdiv(m->D, 256)), dim3(256), 0, st, ta, (const double *)ta.kmat, (const float *)ta.ksum,
             (const double *)ta.ksumd, (const double *)ta.gamma_dev);
  PYZ_LAUNCH_CHECK();
  m->km_valid = false;     // consumed (the next step has another snapshot)
  return PYZ_OK;
}

// phase 2: kernel row(s), repulsion, Adam (SVGD.py:54-68,112-123) on the gradients phase 1 left
static int svgd_sweep_impl(pyz_mlp *m, float *d_particles, int n_local, const float *d_all, int n_total, int row0,
                           float *d_adam_m, float *d_adam_v, float lr, float gamma, int64_t t, int sweep, float *d_loss,
                           hipStream_t st) {
  int rc = svgd_check_rows(m, n_local, n_total, row0, gamma);
  if (rc) return rc;
  if (!d_particles || !d_all || !d_adam_m || !d_adam_v || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (t < 1) return pyz_fail(PYZ_E_INVALID, "Adam step t must be >= 1");
  const bool median = gamma == PYZ_SVGD_GAMMA_MEDIAN;
  if (sweep != PYZ_SWEEP_GAUSS_SEIDEL && sweep != PYZ_SWEEP_JACOBI) return pyz_fail(PYZ_E_INVALID, "unknown sweep %d", sweep);
  if (sweep == PYZ_SWEEP_GAUSS_SEIDEL && (d_all != d_particles || n_local != n_total))
    return pyz_fail(PYZ_E_INVALID, "the Gauss-Seidel sweep needs the whole particle matrix on this device");
  if ((rc = svgd_check_snapshot(m, d_particles, n_local, d_all, n_total, sweep))) return rc;
  if ((rc = svgd_check_gradients(m, n_local))) return rc;
  const int tiles_on = pyz_env_int("PYZ_SVGD_TILES", 1);  // read per call: tests flip it
  const bool tile_ok = sweep == PYZ_SWEEP_JACOBI && svgd_tile_shape(n_local, n_total, row0, d_all, d_particles);
  if (median && !(tile_ok && n_total % 4 == 0))
    return pyz_fail(PYZ_E_INVALID, "the median-heuristic bandwidth needs the Jacobi sweep on a snapshot, at most 64 particles, "
                                   "and particle / local-row counts in multiples of four");
  if (tile_ok && (tiles_on || median)) {
    // every row from the same snapshot: the particle matrix is read once per pass (k_svgd_*_tile)
    if ((rc = svgd_kernel_matrix_impl(m, d_all, n_total, row0, n_local, gamma, nullptr, st))) return rc;
    return svgd_combine_impl(m, d_particles, n_local, d_all, n_total, row0, d_adam_m, d_adam_v, lr, gamma, t, d_loss, st);
  }
  const int nblk = cdiv(m->D, PYZ_SVGD_BLOCK_ELEMS);  // one float64 partial per workgroup of k_svgd_dist
  const int rows_at_once = sweep == PYZ_SWEEP_JACOBI ? n_local : 1;
  if ((rc = need_part2(m, (size_t)rows_at_once * nblk * n_total + 8))) return rc;
  float *loss = m->scal;  // [n_local], written by phase 1
  SvgdArgs a{};
  a.particles = d_particles;
  a.all = d_all;
  a.all_rw = nullptr;
  a.adam_m = d_adam_m;
  a.adam_v = d_adam_v;
  a.grad = m->grad;
  a.D = m->D;
  a.M = n_total;
  a.n_local = n_local;
  a.row0 = row0;
  const double b1t = std::pow(0.9, (double)t), b2t = std::pow(0.999, (double)t);
  a.lr_t = (float)((double)lr * std::sqrt(1.0 - b2t) / (1.0 - b1t));
  a.gamma = gamma;
  a.part = full(m)->x.part2;
  a.nblk = nblk;
  const size_t lds = sizeof(double) * (size_t)(5 * n_total);
  const int jgroups = cdiv(n_total, 8);
  if (sweep == PYZ_SWEEP_JACOBI) {
    a.i_local = -1;
    PYZ_LAUNCH(k_svgd_dist, dim3(nblk, jgroups, n_local), dim3(256), 0, st, a);
    PYZ_LAUNCH(k_svgd_update, dim3(cdiv(m->D, 256), n_local), dim3(256), lds, st, a);
  } else {
    const int gs_fused = pyz_env_int("PYZ_SVGD_GS_FUSED", 1);  // read per call: tests flip it
    const long long gs_range = 256LL * PYZ_GS_E;
    if (gs_fused && n_total <= 64 && m->D <= 256 * gs_range) {
      // one launch per particle, the matrix read once per launch (k_svgd_gs)
      SvgdGsArgs ga{};
      ga.all = d_particles;
      ga.adam_m = d_adam_m;
      ga.adam_v = d_adam_v;
      ga.grad = m->grad;
      ga.D = m->D;
      ga.M = n_total;
      ga.lr_t = a.lr_t;
      ga.gamma = gamma;
      ga.nblk = (int)cdiv(m->D, gs_range);
      const size_t n_part = (size_t)ga.nblk * 64;
      if ((rc = need_part2(m, 2 * n_part + 8))) return rc;
      double *pp[2] = {full(m)->x.part2, full(m)->x.part2 + n_part};
      const size_t gs_lds = pyz_svgd_gs_lds_bytes();
      // (k_svgd_gs's 130 KB of dynamic LDS: allowed when the plan was created, pyz_mlp_create)
      // the whole sweep as ONE resident launch when its workgroups fit the chip at once (k_svgd_gs_resident); read per
      // call: tests flip it
      // workgroups that only sum columns of partials: four columns each in k_svgd_gs_resident, eight in k_svgd_gs_resident2
      const int gs_reducers = pyz_env_int("PYZ_SVGD_GS_RESIDENT", 1) == 2 ? cdiv(n_total, 8) : cdiv(n_total, 4);
      // (1: the partials of row i + 1 through the reducers behind the update of row i; 2: the distances one step early and the
      //  one critical distance in a single hop, k_svgd_gs_resident2)
      const int gs_res_mode = pyz_env_int("PYZ_SVGD_GS_RESIDENT", 1);
      bool resident = gs_res_mode != 0 && ga.nblk + gs_reducers <= pyz_cu_count();
      const void *gs_res_fn = gs_res_mode == 2 ? reinterpret_cast<const void *>(k_svgd_gs_resident2) : reinterpret_cast<const void *>(k_svgd_gs_resident);
      if (resident) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gs_res_fn, 256,
                                                         pyz_svgd_gs_res_lds_bytes()) != hipSuccess || per_cu < 1)
          resident = false;
      }
      if (resident) {
        pyz_mlp_full *fm = full(m);
        const size_t gbytes = 256 + sizeof(unsigned long long) * 2 * (2 * (size_t)256 * 64 + 2 * 64 + 2 * 256);
        const size_t had = fm->x.gs_res_cap;
        if ((rc = ensure_bytes(&fm->x.gs_res_buf, &fm->x.gs_res_cap, gbytes, m))) return rc;
        if (fm->x.gs_res_cap != had)   // a fresh buffer: epoch and tags start at zero (the kernel's tags are >= 1 and only grow)
          PYZ_HIP(hipMemsetAsync(fm->x.gs_res_buf, 0, fm->x.gs_res_cap, st));
        unsigned char *gb = static_cast<unsigned char *>(fm->x.gs_res_buf);
        SvgdGsResArgs ra{};
        ra.all = d_particles;
        ra.adam_m = d_adam_m;
        ra.adam_v = d_adam_v;
        ra.grad = m->grad;
        ra.D = m->D;
        ra.M = n_total;
        ra.lr_t = a.lr_t;
        ra.gamma = gamma;
        ra.nblk = ga.nblk;
        ra.epoch = reinterpret_cast<unsigned *>(gb);
        ra.fail = reinterpret_cast<int *>(gb + 64);
        ra.kgran = reinterpret_cast<unsigned long long *>(gb + 256);
        ra.pgran = ra.kgran + 2 * 64 * 2;
        ra.cgran = ra.pgran + 2 * (size_t)256 * 64 * 2;
        ra.spin_limit = pyz_env_int("PYZ_SVGD_GS_SPIN_LIMIT", 1 << 20);
        if (gs_res_mode == 2) PYZ_LAUNCH(k_svgd_gs_resident2, dim3(ga.nblk + gs_reducers), dim3(256), pyz_svgd_gs_res_lds_bytes(), st, ra);
        else PYZ_LAUNCH(k_svgd_gs_resident, dim3(ga.nblk + gs_reducers), dim3(256), pyz_svgd_gs_res_lds_bytes(), st, ra);
        PYZ_LAUNCH(k_svgd_loss, dim3(1), dim3(64), 0, st, loss, n_local, n_total, d_loss, ra.fail, m->nonfinite);
        PYZ_LAUNCH_CHECK();
        return PYZ_OK;
      }
      const int zigzag = pyz_env_int("PYZ_SVGD_GS_ZIGZAG", 1);   // alternate the row direction from launch to launch (read per call)
      for (int i = -1; i < n_total; ++i) {
        ga.i = i;
        ga.part_in = pp[(i + 2) & 1];   // what launch i - 1 wrote
        ga.part_out = pp[(i + 1) & 1];
        if (zigzag && (i & 1) == 0) PYZ_LAUNCH(k_svgd_gs<true>, dim3(ga.nblk), dim3(256), gs_lds, st, ga);
        else PYZ_LAUNCH(k_svgd_gs<false>, dim3(ga.nblk), dim3(256), gs_lds, st, ga);
      }
    } else {
      for (int i = 0; i < n_local; ++i) {
        a.i_local = i;
        PYZ_LAUNCH(k_svgd_dist, dim3(nblk, jgroups, 1), dim3(256), 0, st, a);
        PYZ_LAUNCH(k_svgd_update, dim3(cdiv(m->D, 256), 1), dim3(256), lds, st, a);
      }
    }
  }
  PYZ_LAUNCH(k_svgd_loss, dim3(1), dim3(64), 0, st, loss, n_local, n_total, d_loss, (int *)nullptr, m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_svgd_gradients(pyz_mlp *m, const float *d_particles, int n_local, const float *d_x, const void *d_y,
                       const int32_t *d_row_idx, int batch, void *stream) {
  return svgd_gradients_impl(m, d_particles, n_local, d_x, d_y, d_row_idx, batch, as_stream(stream));
}

int pyz_svgd_sweep(pyz_mlp *m, float *d_particles, int n_local, const float *d_all, int n_total, int row0,
                   float *d_adam_m, float *d_adam_v, float lr, float gamma, int64_t t, int sweep, float *d_loss,
                   void *stream) {
  return svgd_sweep_impl(m, d_particles, n_local, d_all, n_total, row0, d_adam_m, d_adam_v, lr, gamma, t, sweep, d_loss,
                         as_stream(stream));
}

int pyz_svgd_kernel_matrix(pyz_mlp *m, const float *d_all, int n_total, int row0, int n_local, float gamma, void *stream) {
  return svgd_kernel_matrix_impl(m, d_all, n_total, row0, n_local, gamma, nullptr, as_stream(stream));
}

int pyz_svgd_gram_groups(pyz_mlp *m, const float *d_all, int n_total, int g_lo, int g_hi, double *d_groups, void *stream) {
  return svgd_gram_groups_impl(m, d_all, n_total, g_lo, g_hi, d_groups, as_stream(stream));
}

int pyz_svgd_kernel_matrix_groups(pyz_mlp *m, const double *d_groups, const float *d_all, int n_total, int row0, int n_local,
                                  float gamma, void *stream) {
  if (!d_groups) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  return svgd_kernel_matrix_impl(m, d_all, n_total, row0, n_local, gamma, d_groups, as_stream(stream));
}

int pyz_svgd_combine(pyz_mlp *m, float *d_particles, int n_local, const float *d_all, int n_total, int row0,
                     float *d_adam_m, float *d_adam_v, float lr, float gamma, int64_t t, float *d_loss, void *stream) {
  return svgd_combine_impl(m, d_particles, n_local, d_all, n_total, row0, d_adam_m, d_adam_v, lr, gamma, t, d_loss,
                           as_stream(stream));
}

int pyz_svgd_step(pyz_mlp *m, float *d_particles, int n_local, const float *d_all, int n_total, int row0,
                  float *d_adam_m, float *d_adam_v, const float *d_x, const void *d_y, const int32_t *d_row_idx,
                  int batch, float lr, float gamma, int64_t t, int sweep, float *d_loss, void *stream) {
  // Under the Jacobi sweep d_particles is only written (pyz.h): the rows' current values -- what the gradients are taken
  // at -- are rows [row0, row0 + n_local) of the snapshot
  if (!d_all || !d_particles) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n_total < n_local || row0 < 0 || row0 + n_local > n_total) return pyz_fail(PYZ_E_INVALID, "rows [%d, %d) outside the %d particles", row0, row0 + n_local, n_total);
  if (n_local > 0 && svgd_check_snapshot(m, d_particles, n_local, d_all, n_total, sweep)) return PYZ_E_INVALID;   // (before the gradient pass)
  const float *cur = (sweep == PYZ_SWEEP_JACOBI && d_all != d_particles && m) ? d_all + (long long)row0 * m->D : d_particles;
  const int rc = svgd_gradients_impl(m, cur, n_local, d_x, d_y, d_row_idx, batch, as_stream(stream));
  if (rc) return rc;
  return svgd_sweep_impl(m, d_particles, n_local, d_all, n_total, row0, d_adam_m, d_adam_v, lr, gamma, t, sweep, d_loss,
                         as_stream(stream));
}

// ---------------------------------------------------------------- R1
int pyz_predict(pyz_mlp *m, const float *d_weights, int n_samples, const float *d_x, int n, float *d_samples,
                float *d_mean, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (n_samples <= 0 || n <= 0) return pyz_fail(PYZ_E_INVALID, "n_samples and n must be positive");
  if (n > m->max_batch) return pyz_fail(PYZ_E_SHAPE, "n %d exceeds the plan's max_batch %d", n, m->max_batch);
  if (!d_weights || !d_x || !d_mean) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  return net_predict(Net{nullptr, m}, d_weights, n_samples, d_x, n, d_samples, d_mean, stream);
}

int pyz_predict_moments(pyz_mlp *m, const float *d_weights, int n_samples, const float *d_x, int n, float *d_mean,
                        float *d_m2, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (n_samples <= 0 || n <= 0) return pyz_fail(PYZ_E_INVALID, "n_samples and n must be positive");
  if (n > m->max_batch) return pyz_fail(PYZ_E_SHAPE, "n %d exceeds the plan's max_batch %d", n, m->max_batch);
  if (!d_weights || !d_x || !d_mean || !d_m2) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  return net_predict_moments(Net{nullptr, m}, d_weights, n_samples, d_x, n, d_mean, d_m2, stream);
}

// ---------------------------------------------------------------- decision surfaces (Plotter)
int pyz_grid_rows(const float *d_basis, int d, float a0, float da, int n1, float b0, float db, int n2, int64_t row0,
                  int64_t n, float *d_out, void *stream) {
  if (n1 < 1 || n2 < 1 || d < 1) return pyz_fail(PYZ_E_INVALID, "n1, n2 and d must be positive");
  const int64_t total = (int64_t)n1 * n2;
  if (row0 < 0 || n < 1 || row0 > total || n > total - row0)
    return pyz_fail(PYZ_E_INVALID, "rows [%lld, %lld) outside the %d x %d grid", (long long)row0, (long long)(row0 + n), n1, n2);
  if (!d_basis || !d_out) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  const long long n_out = (long long)n * d;
  if (cdiv(n_out, 256) > 0x7fffffffLL) return pyz_fail(PYZ_E_INVALID, "too many rows for one call: split the row range");
  PYZ_LAUNCH(k_grid_rows, dim3((unsigned)cdiv(n_out, 256)), dim3(256), 0, as_stream(stream), d_basis, d, a0, da, b0, db, n2,
             (long long)row0, n_out, d_out);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_predict_surface(pyz_mlp *m, const float *d_weights, int n_samples, const float *d_x, int n, int column,
                        float *d_cols, float *d_mean, float *d_top, int32_t *d_cls, float *d_ent, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (n_samples < 1 || n < 1) return pyz_fail(PYZ_E_INVALID, "n_samples and n must be positive");
  if (n > m->max_batch) return pyz_fail(PYZ_E_SHAPE, "n %d exceeds the plan's max_batch %d", n, m->max_batch);
  PredictSurfaceArgs g{};
  g.C = m->dims[m->L];
  if (column < 0 || column >= g.C) return pyz_fail(PYZ_E_INVALID, "column %d outside [0, %d)", column, g.C);
  if (!d_weights || !d_x || !d_mean) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (!pyz_predict_surface_fits(g.C))
    return pyz_fail(PYZ_E_SHAPE, "a row of %d outputs does not fit the surface kernel's LDS", g.C);
  hipStream_t st = as_stream(stream);
  int rc = set_ctl(m, 0, n, 0.0f, 0, 0, 0, st);
  if (rc) return rc;
  g.last = m->act[m->L - 1];
  g.pstride = (long long)m->max_batch * g.C;
  g.softmax = m->acts[m->L - 1] == PYZ_ACT_SOFTMAX ? 1 : 0;
  g.n = n;
  g.column = column;
  g.mean = d_mean;
  g.top = d_top;
  g.cls = d_cls;
  g.ent = d_ent;
  g.inv_total = 1.0f / (float)n_samples;
  return for_draw_chunks(Net{nullptr, m}, d_weights, n_samples, d_x, n, m->max_p, st, [&](int s0, int S, const float *) {
    g.S = S;
    g.accumulate = s0 > 0 ? 1 : 0;
    g.finish = s0 + S >= n_samples && (d_top || d_cls || d_ent) ? 1 : 0;
    g.cols = d_cols ? d_cols + (long long)s0 * n : nullptr;
    if (!pyz_launch_predict_surface(g, st))
      return pyz_fail(PYZ_E_SHAPE, "a row of %d outputs does not fit the surface kernel's LDS", g.C);
    return PYZ_OK;
  });
}

// ---------------------------------------------------------------- R2
int pyz_input_grad(pyz_mlp *m, const float *d_weights, int n_samples, const float *d_x, const void *d_y, int n, float scale,
                   float *d_xgrad, float epsilon, float *d_xadv, float *d_loss, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (n_samples < 1 || n < 1) return pyz_fail(PYZ_E_INVALID, "n_samples and n must be positive");
  if (n > m->max_batch) return pyz_fail(PYZ_E_SHAPE, "n %d exceeds the plan's max_batch %d", n, m->max_batch);
  int rc = check_loss_combo(m);
  if (rc) return rc;
  if (!d_weights || !d_x || !d_y || !d_xgrad) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  hipStream_t st = as_stream(stream);
  if ((rc = set_ctl(m, 0, n, 0.0f, 0, 0, 0, st))) return rc;
  m->grad_owner = 2;   // (the losses of a call without d_loss land in m->scal)
  const int N = m->dims[1];
  const int chunk = std::min(m->max_p, pyz_input_grad_max_draws(N));
  // (no forward from the walk: launch_delta0 runs the one its head needs)
  return for_draw_chunks(Net{nullptr, m}, d_weights, n_samples, d_x, n, chunk, st, [&](int s0, int P, const float *theta) {
    launch_delta0(m, theta, P, d_x, d_y, n, st);
    PYZ_LAUNCH(k_loss_finalize, dim3(P), dim3(64), 0, st, m->part, m->cur_nblk, m->ctl, d_loss ? d_loss + s0 : m->scal,
               m->nonfinite);
    InputGradArgs g{};
    g.delta = m->delta[0];
    g.delta_pstride = (long long)m->max_batch * N;
    g.theta = theta;
    g.theta_pstride = m->D;
    g.w_off = m->w_off[0];
    g.K = m->dims[0];
    g.N = N;
    g.P = P;
    g.rows = n;
    g.vec = (N % 8 == 0) && (m->w_off[0] % 4 == 0) && (P == 1 || m->D % 4 == 0) && aligned16(theta) ? 1 : 0;
    g.scale = scale;
    g.out = d_xgrad;
    g.accumulate = s0 > 0 ? 1 : 0;
    if (d_xadv && s0 + P >= n_samples) {   // the last chunk: G is complete in its epilogue
      g.x = d_x;
      g.xadv = d_xadv;
      g.eps = epsilon;
    }
    pyz_launch_input_grad(g, st);
    return PYZ_OK;
  }, false);
}

// ---------------------------------------------------------------- noise
int pyz_sample_normal_rows(float *d_out, int64_t n_rows, int64_t row_stride, int64_t col0, int64_t len, const float *d_loc,
                           const float *d_scale, uint64_t seed, uint32_t stream_id, uint32_t first_draw, void *stream) {
  if (!d_out || !d_loc || !d_scale) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n_rows <= 0 || n_rows > 65535 || len <= 0 || col0 < 0 || col0 + len > row_stride)
    return pyz_fail(PYZ_E_INVALID, "bad draw count / column range");
  PYZ_LAUNCH(k_sample_normal_rows, dim3(cdiv(cdiv(len, 4), 256), (unsigned)n_rows), dim3(256), 0, as_stream(stream), d_out,
                     (long long)row_stride, (long long)col0, (long long)len, d_loc, d_scale, seed, stream_id, first_draw);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_sample_lowrank_rows(float *d_out, int64_t n_rows, int64_t row_stride, int64_t col0, int64_t len, const float *d_mean,
                            const float *d_diag, const float *d_dev, int k, float factor, uint64_t seed, uint32_t stream_id,
                            uint32_t first_draw, void *stream) {
  if (!d_out || !d_mean || !d_diag || !d_dev) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n_rows <= 0 || n_rows > 65535 || len <= 0 || col0 < 0 || col0 + len > row_stride)
    return pyz_fail(PYZ_E_INVALID, "bad draw count / column range");
  if (k < 1 || k > PYZ_LOWRANK_MAX_K)
    return pyz_fail(PYZ_E_INVALID, "k %d outside [1, %d] (PYZ_LOWRANK_MAX_K)", k, PYZ_LOWRANK_MAX_K);
  const int vec_in = aligned16(d_mean) && aligned16(d_diag) && aligned16(d_dev) && (len % 4 == 0 || k == 1) ? 1 : 0;
  PYZ_LAUNCH(k_sample_lowrank_rows, dim3(cdiv(len, PYZ_LOWRANK_TILE), cdiv(n_rows, PYZ_LOWRANK_ROWS)), dim3(256), 0,
             as_stream(stream), d_out, (int)n_rows, (long long)row_stride, (long long)col0, (long long)len, d_mean, d_diag, d_dev,
             k, factor, vec_in, seed, stream_id, first_draw);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_gather_rows(float *d_out, int64_t n_rows, int64_t row_stride, int64_t col0, int64_t len, const float *d_bank,
                    int64_t n_bank, const int32_t *d_idx, void *stream) {
  if (!d_out || !d_bank || !d_idx) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n_rows <= 0 || n_rows > 65535 || len <= 0 || col0 < 0 || col0 + len > row_stride)
    return pyz_fail(PYZ_E_INVALID, "bad row count / column range");
  if (n_bank < 1) return pyz_fail(PYZ_E_INVALID, "the bank must hold at least one row");
  PYZ_LAUNCH(k_gather_rows, dim3(cdiv(cdiv(len, 4), 256), (unsigned)n_rows), dim3(256), 0, as_stream(stream), d_out,
             (long long)row_stride, (long long)col0, (long long)len, d_bank, (long long)n_bank, d_idx);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_fill_normal(float *d_out, int64_t n, uint64_t seed, uint32_t stream_id, uint32_t step, float mean, float std,
                    void *stream) {
  if (!d_out || n <= 0) return pyz_fail(PYZ_E_INVALID, "bad output buffer");
  PYZ_LAUNCH(k_fill_normal, dim3(cdiv(cdiv(n, 4), 256)), dim3(256), 0, as_stream(stream), d_out, (long long)n,
                     seed, stream_id, step, mean, std);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- corrupted read-outs (no plan)
int pyz_corrupt_rows(const float *d_x, int64_t n, int h, int w, int ch, int kind, const int32_t *severities, int n_sev,
                     float pixel_max, int quantise, uint64_t seed, float *d_out, void *stream) {
  if (kind < 0 || kind >= PYZ_CORRUPT_KINDS) return pyz_fail(PYZ_E_INVALID, "unknown corruption kind %d", kind);
  if (!severities || n_sev < 1 || n_sev > PYZ_CORRUPT_MAX_SEV)
    return pyz_fail(PYZ_E_INVALID, "n_sev %d outside 1..%d", n_sev, PYZ_CORRUPT_MAX_SEV);
  if (n < 1 || n > INT_MAX || h < 1 || w < 1) return pyz_fail(PYZ_E_INVALID, "n, h and w must be positive (n below 2^31)");
  CorruptArgs g{};
  size_t lds = 0;
  if (kind == PYZ_CORRUPT_REGRESSION) {
    if (h != 1 || ch != 1) return pyz_fail(PYZ_E_INVALID, "the regression noise takes rows: h = ch = 1, the length as w");
  } else {
    if (ch != 1 && ch != 3) return pyz_fail(PYZ_E_INVALID, "ch %d: an image has 1 or 3 channels", ch);
    if (!(pixel_max > 0.0f)) return pyz_fail(PYZ_E_INVALID, "pixel_max must be positive");
    if ((long long)h * w > PYZ_LDS_BYTES / 24 || pyz_corrupt_lds(h, w) > PYZ_LDS_BYTES)
      return pyz_fail(PYZ_E_INVALID, "a %d x %d image and its scratch copy (three channels each) do not fit %d KiB of LDS", h, w,
                      PYZ_LDS_BYTES / 1024);
    if (kind == PYZ_C_BLUR || kind == PYZ_C_CONTRAST || kind == PYZ_C_PIXELATE) lds = pyz_corrupt_lds(h, w);
  }
  g.kind = kind;
  g.h = h;
  g.w = w;
  g.ch = ch;
  g.planes = ch;
  int rc = pyz_corrupt_tables(g, severities, n_sev);
  if (rc) return rc;
  if (!d_x || !d_out) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  g.x = d_x;
  g.out = d_out;
  g.n = n;
  g.pixel_max = pixel_max;
  g.quantise = quantise ? 1 : 0;
  g.out_scale = g.quantise ? pixel_max / 255.0f : pixel_max;
  g.seed = seed;
  if (lds > 64 * 1024)
    PYZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_corrupt_rows), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  PYZ_LAUNCH(k_corrupt_rows, dim3((unsigned)n, (unsigned)n_sev), dim3(PYZ_CORRUPT_THREADS), lds, as_stream(stream), g);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_score_rows(const float *d_mean, int groups, int64_t n, int C, const void *d_y, int kind, void *d_out, void *stream) {
  if (kind != 0 && kind != 1) return pyz_fail(PYZ_E_INVALID, "kind %d: 0 = classification, 1 = regression", kind);
  if (groups < 1 || groups > 65535 || n < 1 || C < 1) return pyz_fail(PYZ_E_INVALID, "groups (at most 65535), n and C must be positive");
  if (!d_mean || !d_y || !d_out) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  hipStream_t st = as_stream(stream);
  if (kind == 0) {
    PYZ_HIP(hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * groups, st));
    PYZ_LAUNCH(k_score_rows, dim3((unsigned)cdiv(n, 256), (unsigned)groups), dim3(256), 0, st, d_mean, (long long)n, C, d_y, 0,
               static_cast<unsigned long long *>(d_out), (double *)nullptr);
  } else {
    const long long nblk = cdiv(n, PYZ_SCORE_ROWS_PER_BLOCK), total = (long long)groups * C;
    if (total > INT_MAX || nblk > INT_MAX) return pyz_fail(PYZ_E_INVALID, "groups * C and the row blocks must stay below 2^31");
    double *part = nullptr;   // the per-workgroup sums: stream-ordered scratch, gone when k_score_sum has read it
    PYZ_HIP(hipMallocAsync((void **)&part, sizeof(double) * (size_t)total * (size_t)nblk, st));
    PYZ_LAUNCH(k_score_rows, dim3((unsigned)nblk, (unsigned)groups), dim3(256), 0, st, d_mean, (long long)n, C, d_y, 1,
               (unsigned long long *)nullptr, part);
    PYZ_LAUNCH(k_score_sum, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, (const double *)part, (int)nblk, (int)total,
               static_cast<double *>(d_out));
    PYZ_HIP(hipFreeAsync(part, st));
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- D1: Deep-PILCO policy update (pyz_pilco.h)
struct pyz_pilco {
  PilcoArgs a{};                 // the nets, K, S, A and the workspace pointers; the per-call fields are filled by each call
  int max_h = 0;
  void *ws = nullptr;            // one allocation: the tape, the state gradients, the partial rows, the call's scalars
  size_t ws_bytes = 0;
  float *st_own = nullptr, *ac_own = nullptr;   // states / actions when the caller does not ask for them
  PilcoCtl *ctl = nullptr;
  PyzGraphCache<4> graphs;       // one graph per (H, freq); everything else baked into them is the cache's key
};

// kinds / gammas: one entry per layer, or null: every layer Dense
static int pilco_net(PilcoNet &net, const char *what, int L, const int32_t *dims, const int32_t *acts, bool softmax_last,
                     const int32_t *kinds, const float *gammas) {
  if (!dims || !acts || (kinds && !gammas)) return pyz_fail(PYZ_E_INVALID, "null argument");
  if (L < 1 || L > PILCO_MAX_LAYERS) return pyz_fail(PYZ_E_INVALID, "%s: %d layers outside [1, %d]", what, L, PILCO_MAX_LAYERS);
  net.L = L;
  int off = 0;
  for (int l = 0; l <= L; ++l) {
    if (dims[l] < 1 || dims[l] > PILCO_MAX_WIDTH)
      return pyz_fail(PYZ_E_INVALID, "%s: dims[%d] = %d outside [1, %d]", what, l, dims[l], PILCO_MAX_WIDTH);
    net.dims[l] = dims[l];
  }
  for (int l = 0; l < L; ++l) {
    const bool last = l == L - 1;
    const int kind = kinds ? kinds[l] : PYZ_PILCO_DENSE;
    if (kind != PYZ_PILCO_DENSE && kind != PYZ_PILCO_RBF) return pyz_fail(PYZ_E_INVALID, "%s: unknown kind %d of layer %d", what, kind, l);
    if (acts[l] < PYZ_ACT_LINEAR || acts[l] > PYZ_ACT_SOFTMAX || (acts[l] == PYZ_ACT_SOFTMAX && !(last && softmax_last)))
      return pyz_fail(PYZ_E_INVALID, "%s: activation %d at layer %d is not supported", what, acts[l], l);
    net.acts[l] = acts[l];
    net.kind[l] = kind;
    net.gamma[l] = 0.0f;
    net.w_off[l] = off;
    if (kind == PYZ_PILCO_RBF) {
      if (last) return pyz_fail(PYZ_E_INVALID, "%s: an RBF layer cannot be the last layer", what);
      if (!std::isfinite(gammas[l]) || !(gammas[l] > 0.0f))
        return pyz_fail(PYZ_E_INVALID, "%s: gamma %g of RBF layer %d is not a finite number > 0", what, (double)gammas[l], l);
      if (acts[l] != PYZ_ACT_LINEAR) return pyz_fail(PYZ_E_INVALID, "%s: RBF layer %d takes no activation (pass linear)", what, l);
      net.gamma[l] = gammas[l];
      off += dims[l] * dims[l + 1];                  // the means: no bias
    } else {
      off += (dims[l] + 1) * dims[l + 1];
    }
  }
  return PYZ_OK;
}

int pyz_pilco_create(int n_policy_layers, const int32_t *h_policy_dims, const int32_t *h_policy_acts, int n_dynamics_layers,
                     const int32_t *h_dynamics_dims, const int32_t *h_dynamics_acts, int particles, int max_horizon,
                     pyz_pilco **out) {
  int32_t kinds[PILCO_MAX_LAYERS];                 // (pilco_net reads the first n_policy_layers, once it has checked that count)
  float gammas[PILCO_MAX_LAYERS];
  for (int l = 0; l < PILCO_MAX_LAYERS; ++l) {
    kinds[l] = PYZ_PILCO_DENSE;
    gammas[l] = 0.0f;
  }
  return pyz_pilco_create_layers(n_policy_layers, h_policy_dims, h_policy_acts, kinds, gammas, n_dynamics_layers, h_dynamics_dims,
                                 h_dynamics_acts, particles, max_horizon, out);
}

int pyz_pilco_create_layers(int n_policy_layers, const int32_t *h_policy_dims, const int32_t *h_policy_acts,
                            const int32_t *h_policy_kinds, const float *h_policy_gammas, int n_dynamics_layers,
                            const int32_t *h_dynamics_dims, const int32_t *h_dynamics_acts, int particles, int max_horizon,
                            pyz_pilco **out) {
  if (!out) return pyz_fail(PYZ_E_INVALID, "null argument");
  *out = nullptr;
  if (!h_policy_kinds || !h_policy_gammas) return pyz_fail(PYZ_E_INVALID, "null argument");
  PilcoArgs a{};
  int rc;
  if ((rc = pilco_net(a.pol, "policy", n_policy_layers, h_policy_dims, h_policy_acts, true, h_policy_kinds, h_policy_gammas))) return rc;
  if ((rc = pilco_net(a.dyn, "dynamics", n_dynamics_layers, h_dynamics_dims, h_dynamics_acts, false, nullptr, nullptr))) return rc;
  if (a.dyn.acts[a.dyn.L - 1] != PYZ_ACT_LINEAR)
    return pyz_fail(PYZ_E_INVALID, "the dynamics' last layer must be linear, not activation %d", a.dyn.acts[a.dyn.L - 1]);
  if (particles < 2 || particles > PILCO_MAX_K)
    return pyz_fail(PYZ_E_INVALID, "%d particles outside [2, %d] (one particle has deviation 0 and a NaN gradient)", particles, PILCO_MAX_K);
  if (max_horizon < 1 || max_horizon > PILCO_MAX_H) return pyz_fail(PYZ_E_INVALID, "max_horizon %d outside [1, %d]", max_horizon, PILCO_MAX_H);
  const int S = a.pol.dims[0], A = a.pol.dims[a.pol.L];
  if (S + A > PILCO_MAX_IN) return pyz_fail(PYZ_E_INVALID, "S + A = %d exceeds %d", S + A, PILCO_MAX_IN);
  if (a.dyn.dims[0] != S + A || a.dyn.dims[a.dyn.L] != S)
    return pyz_fail(PYZ_E_INVALID, "dynamics dims (%d -> %d) do not fit the policy's (S = %d, A = %d): expected %d -> %d",
                    a.dyn.dims[0], a.dyn.dims[a.dyn.L], S, A, S + A, S);
  const int K = particles;
  a.K = K;
  a.S = S;
  a.A = A;
  a.Dp = a.pol.w_off[a.pol.L - 1] + (long long)(a.pol.dims[a.pol.L - 1] + 1) * A;
  a.Dd = a.dyn.w_off[a.dyn.L - 1] + (long long)(a.dyn.dims[a.dyn.L - 1] + 1) * S;
  a.maxw = PILCO_MAX_IN;
  for (int l = 0; l <= a.pol.L; ++l) a.maxw = std::max(a.maxw, a.pol.dims[l]);
  for (int l = 0; l <= a.dyn.L; ++l) a.maxw = std::max(a.maxw, a.dyn.dims[l]);
  for (int l = 1; l < a.pol.L; ++l) a.tw_pol += a.pol.dims[l];
  a.tw = a.tw_pol;
  for (int l = 1; l < a.dyn.L; ++l) a.tw += a.dyn.dims[l];
  a.pw = S + a.tw_pol + A;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return pyz_fail(PYZ_E_NODEV, "no HIP device visible");

  // workspace, in floats (each block rounded up to 64): y H K S + states (H + 1) K S + actions H K A + tape H K tw +
  // (m, sd) 2 H S + state gradients 2 K S + rewards (H + 1) K + cost factors H + 1 + partial rows K D_pol +
  // transposed kernels K D_dyn + D_pol + 64 for the scalars
  const size_t Hm = (size_t)max_horizon, KS = (size_t)K * S;
  const size_t n[] = {Hm * KS, (Hm + 1) * KS, Hm * K * A, Hm * K * (size_t)a.tw, 2 * Hm * S, 2 * KS, (Hm + 1) * K, Hm + 1,
                      (size_t)K * (size_t)a.Dp, (size_t)K * (size_t)a.Dd, (size_t)a.Dp, 64};
  size_t total = 0;
  for (size_t v : n) total += (v + 63) & ~(size_t)63;
  pyz_pilco *p = new pyz_pilco();
  p->ws_bytes = total * sizeof(float);
  if (hipMalloc(&p->ws, p->ws_bytes) != hipSuccess) {
    const size_t bytes = p->ws_bytes;
    delete p;
    return pyz_fail(PYZ_E_OOM, "workspace allocation of %zu bytes failed", bytes);
  }
  float *base = static_cast<float *>(p->ws);
  float **slot[] = {&a.y, &p->st_own, &p->ac_own, &a.tape, &a.msd, &a.g, &a.rew, &a.coef, &a.part, &a.WT, &a.phiT};
  for (int q = 0; q < 11; ++q) {
    *slot[q] = base;
    base += (n[q] + 63) & ~(size_t)63;
  }
  p->ctl = reinterpret_cast<PilcoCtl *>(base);
  a.ctl = p->ctl;
  p->a = a;
  p->max_h = max_horizon;
  const size_t lds = std::max(pilco_fwd_lds(K, S, a.maxw), pilco_bwd_lds(K, S, a.maxw, a.pw));
  if (lds > 160 * 1024) {
    pyz_pilco_destroy(p);
    return pyz_fail(PYZ_E_INVALID, "the step kernels would need %zu bytes of LDS", lds);
  }
  if (lds > 64 * 1024)
    for (const void *k : {reinterpret_cast<const void *>(k_pilco_fwd), reinterpret_cast<const void *>(k_pilco_tail),
                          reinterpret_cast<const void *>(k_pilco_bwd)})
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        pyz_pilco_destroy(p);
        return pyz_fail(PYZ_E_HIP, "hipFuncSetAttribute(k_pilco_*) failed");
      }
  *out = p;
  return PYZ_OK;
}

int pyz_pilco_destroy(pyz_pilco *p) {
  if (!p) return PYZ_OK;
  p->graphs.drop();
  if (p->ws) (void)hipFree(p->ws);
  delete p;
  return PYZ_OK;
}

int64_t pyz_pilco_workspace_bytes(const pyz_pilco *p) { return p ? (int64_t)p->ws_bytes : -1; }

int pyz_pilco_policy_step(pyz_pilco *p, float *d_phi, float *d_m, float *d_v, int64_t adam_t, const float *d_W,
                          const float *d_s0, const float *d_eps, int H, int freq, float gamma, int reward, float lr,
                          float *d_cost, float *d_grad, float *d_states, float *d_actions, int use_graph, void *stream) {
  if (!p) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (H < 1 || H > p->max_h) return pyz_fail(PYZ_E_SHAPE, "horizon %d outside [1, %d] of the plan", H, p->max_h);
  if (freq < 1) return pyz_fail(PYZ_E_INVALID, "freq %d must be >= 1", freq);
  if (reward != PYZ_REWARD_CART && reward != PYZ_REWARD_ACB) return pyz_fail(PYZ_E_INVALID, "unknown reward %d", reward);
  const int need = reward == PYZ_REWARD_CART ? 4 : 5;
  if (p->a.S < need) return pyz_fail(PYZ_E_INVALID, "reward %d reads %d state entries, the state has %d", reward, need, p->a.S);
  if (adam_t < 0) return pyz_fail(PYZ_E_INVALID, "adam_t %lld must be >= 0", (long long)adam_t);
  if (!d_phi || !d_W || !d_s0 || !d_eps || !d_cost || !d_grad || (adam_t > 0 && (!d_m || !d_v)))
    return pyz_fail(PYZ_E_INVALID, "null device pointer");
  hipStream_t st = as_stream(stream);
  PilcoArgs a = p->a;
  a.H = H;
  a.reward = reward;
  a.phi = d_phi;
  a.phi_out = d_phi;
  a.m = d_m;
  a.v = d_v;
  a.W = d_W;
  a.s0 = d_s0;
  a.eps = d_eps;
  a.cost = d_cost;
  a.grad = d_grad;
  a.st = d_states ? d_states : p->st_own;
  a.ac = d_actions ? d_actions : p->ac_own;

  // the scalars of this call: not part of a captured graph
  float lr_t = 0.0f;
  if (adam_t > 0) lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow(0.999, (double)adam_t)) / (1.0 - std::pow(0.9, (double)adam_t)));
  auto tiles = [](const PilcoNet &net) {
    int n = 0;
    for (int l = 0; l < net.L; ++l) n += cdiv(net.dims[l], 32) * cdiv(net.dims[l + 1], 32);
    return n;
  };
  PYZ_LAUNCH(k_pilco_set, dim3(std::max({tiles(a.pol), tiles(a.dyn), cdiv(H + 1, 256)}), a.K + 2), dim3(256), 0, st, a, p->ctl,
             freq, (double)gamma, lr_t, adam_t > 0 ? 1 : 0);
  PYZ_LAUNCH_CHECK();

  const size_t lds_f = pilco_fwd_lds(a.K, a.S, a.maxw), lds_b = pilco_bwd_lds(a.K, a.S, a.maxw, a.pw);
  auto chain = [&]() {
    PilcoArgs g = a;
    for (int t = 1; t <= H; ++t) {
      g.t = t;
      PYZ_LAUNCH(k_pilco_fwd, dim3(a.K), dim3(PILCO_THREADS), lds_f, st, g);
    }
    g.t = H + 1;
    PYZ_LAUNCH(k_pilco_tail, dim3(a.K), dim3(PILCO_THREADS), lds_f, st, g);
    for (int t = H; t >= 1; --t) {
      g.t = t;
      PYZ_LAUNCH(k_pilco_bwd, dim3(a.K), dim3(PILCO_THREADS), lds_b, st, g);
    }
    PYZ_LAUNCH(k_pilco_close, dim3(cdiv(a.Dp, 256)), dim3(256), 0, st, g);
    PYZ_LAUNCH_CHECK();
    return PYZ_OK;
  };
  if (!use_graph || st == nullptr || pyz_probe().on) return chain();   // (the legacy default stream cannot be captured)
  unsigned long long key = 1469598103934665603ull;
  auto mix = [&](unsigned long long v) { key = (key ^ v) * 1099511628211ull; };
  for (const void *q : {(const void *)d_phi, (const void *)d_m, (const void *)d_v, (const void *)d_W, (const void *)d_s0,
                        (const void *)d_eps, (const void *)d_cost, (const void *)d_grad, (const void *)a.st, (const void *)a.ac})
    mix((unsigned long long)(uintptr_t)q);
  mix((unsigned long long)reward);
  p->graphs.rekey(key);
  p->graphs.begin_call();
  return p->graphs.launch(H, (unsigned long long)freq, 0, 4, st, chain);
}

int pyz_pilco_act(pyz_pilco *p, const float *d_phi, const float *d_states, int N, float *d_actions, void *stream) {
  if (!p) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (N < 1) return pyz_fail(PYZ_E_INVALID, "%d state rows: at least one is needed", N);
  if (!d_phi || !d_states || !d_actions) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  PilcoArgs a = p->a;
  a.phi = d_phi;
  PYZ_LAUNCH(k_pilco_act, dim3(N), dim3(PILCO_THREADS), pilco_act_lds(a.maxw), as_stream(stream), a, d_states, d_actions);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- measurement hook
int pyz_bench_dense_kernel(pyz_mlp *m, int kind, int layer, const float *d_theta, int P, const float *d_x,
                           const int32_t *d_row_idx, int batch, float *d_grad, int iters, void *stream) {
  int rc = check_call(m, P, batch);
  if (rc) return rc;
  if (layer < 0 || layer >= m->L || kind < 0 || kind > 2 || iters < 1) return pyz_fail(PYZ_E_INVALID, "bad kind/layer/iters");
  if (kind == 1 && layer == 0) return pyz_fail(PYZ_E_INVALID, "layer 0 has no data gradient");
  if (!d_theta || !d_x || (kind == 2 && !d_grad)) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  hipStream_t st = as_stream(stream);
  if ((rc = set_ctl(m, 0, batch, 0.0f, 0, 0, 0, st))) return rc;
  const int K = m->dims[layer], N = m->dims[layer + 1];
  DenseArgs g{};
  g.K = K;
  g.N = N;
  g.theta = d_theta;
  g.theta_pstride = m->D;
  g.w_off = m->w_off[layer];
  g.ctl = m->ctl;
  if (kind == 1) {
    g.in = m->delta[layer];
    g.in_pstride = (long long)m->max_batch * N;
    g.lda = N;
    g.out = m->delta[layer - 1];
    g.out_pstride = (long long)m->max_batch * K;
    g.aux = m->act[layer - 1];
    g.aux_pstride = (long long)m->max_batch * K;
    g.act = m->acts[layer - 1];
    g.vec = (N % 8 == 0) && (m->w_off[layer] % 4 == 0) && (P == 1 || m->D % 4 == 0) && aligned16(d_theta) ? 1 : 0;
  } else if (kind == 0) {
    if (layer == 0) {
      g.in = d_x;
      g.in_pstride = 0;
      g.row_idx = d_row_idx;
    } else {
      g.in = m->act[layer - 1];
      g.in_pstride = (long long)m->max_batch * K;
    }
    g.lda = K;
    g.out = m->act[layer];
    g.out_pstride = (long long)m->max_batch * N;
    g.act = m->acts[layer];
    g.vec = (K % 8 == 0) && aligned16(g.in) ? 1 : 0;
  }
  WgradArgs u{};
  u.mode = PYZ_UPD_NONE;
  u.grad = d_grad;
  u.grad_pstride = m->D;
  for (int i = 0; i < iters; ++i) {
    if (kind == 0) {
      if (!pyz_launch_fwd_ring(g, batch, P, st)) pyz_launch_fwd(g, batch, P, st);
    }
    else if (kind == 1) pyz_launch_bwd_data(g, batch, P, st);
    else launch_wgrad_all(m, P, d_x, d_row_idx, batch, m->ctl, u, st, nullptr);  // the launch the step uses (all layers)
  }
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

// ---------------------------------------------------------------- per-launch timing
int pyz_probe_begin(int max_launches) {
  if (max_launches < 1 || max_launches > (1 << 20)) return pyz_fail(PYZ_E_INVALID, "max_launches outside [1, 2^20]");
  PyzProbe &p = pyz_probe();
  if (p.on) return pyz_fail(PYZ_E_INVALID, "a probe is already open on this thread");
  while ((int)p.ev.size() < 2 * max_launches) {
    hipEvent_t e = nullptr;
    PYZ_HIP(hipEventCreate(&e));
    p.ev.push_back(e);
  }
  p.name.assign((size_t)max_launches, nullptr);
  p.cap = max_launches;
  p.n = 0;
  p.on = true;
  return PYZ_OK;
}

int pyz_probe_end(void *stream, float *h_us, char *h_names, int name_stride, int *h_n) {
  PyzProbe &p = pyz_probe();
  if (!p.on) return pyz_fail(PYZ_E_INVALID, "no probe open on this thread");
  p.on = false;
  if (!h_us || !h_n) return pyz_fail(PYZ_E_INVALID, "null pointer");
  PYZ_HIP(hipStreamSynchronize(as_stream(stream)));
  for (int i = 0; i < p.n; ++i) {
    float ms = 0.0f;
    PYZ_HIP(hipEventElapsedTime(&ms, p.ev[2 * i], p.ev[2 * i + 1]));
    h_us[i] = ms * 1e3f;
    if (h_names && name_stride > 1) {
      const char *nm = p.name[i] ? p.name[i] : "";
      const bool wrapped = nm[0] == '(';  // "(k_head_rows<4, 12>)": the launch site wraps template kernels in parentheses
      char *dst = h_names + (size_t)i * name_stride;
      std::snprintf(dst, (size_t)name_stride, "%s", nm + (wrapped ? 1 : 0));
      const size_t len = std::strlen(dst);
      if (wrapped && len > 0 && dst[len - 1] == ')') dst[len - 1] = '\0';
    }
  }
  *h_n = p.n;
  return PYZ_OK;
}

int pyz_last_run_info(const pyz_mlp *m, int32_t *h_graph_steps, int32_t *h_eager_steps, int32_t *h_graph_launches) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (h_graph_steps) *h_graph_steps = m->run_graph_steps;
  if (h_eager_steps) *h_eager_steps = m->run_eager_steps;
  if (h_graph_launches) *h_graph_launches = m->run_graph_launches;
  return PYZ_OK;
}

int pyz_run_batch_form(const pyz_mlp *m, int32_t *h_form) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (h_form) *h_form = m->run_batch_form;
  return PYZ_OK;
}

int pyz_sgld_run_info(const pyz_mlp *m, int32_t *h_captures) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (h_captures) *h_captures = m->graphs.captures;
  return PYZ_OK;
}

// ---------------------------------------------------------------- non-finite sentinel
int pyz_check_finite(pyz_mlp *m, void *stream) {
  if (!m) return pyz_fail(PYZ_E_INVALID, "null plan");
  hipStream_t st = as_stream(stream);
  int n = 0;
  PYZ_HIP(hipMemcpyAsync(&n, m->nonfinite, sizeof n, hipMemcpyDeviceToHost, st));
  PYZ_HIP(hipMemsetAsync(m->nonfinite, 0, sizeof n, st));
  PYZ_HIP(hipStreamSynchronize(st));
  if (n > 0) return pyz_fail(PYZ_E_NAN, "%d step(s) since the last check produced a NaN / Inf loss", n);
  return PYZ_OK;
}

// ---------------------------------------------------------------- memory of callers without a device allocator
int pyz_malloc(size_t bytes, void **d_out) {
  if (!d_out || bytes == 0) return pyz_fail(PYZ_E_INVALID, "bad allocation request");
  *d_out = nullptr;
  PYZ_HIP(hipMalloc(d_out, bytes));
  return PYZ_OK;
}

int pyz_free(void *d_ptr) {
  if (d_ptr) PYZ_HIP(hipFree(d_ptr));
  return PYZ_OK;
}

int pyz_upload(void *d_dst, const void *h_src, size_t bytes, void *stream) {
  if (!d_dst || !h_src) return pyz_fail(PYZ_E_INVALID, "null pointer");
  PYZ_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, as_stream(stream)));
  PYZ_HIP(hipStreamSynchronize(as_stream(stream)));  // the host buffer is the caller's again on return
  return PYZ_OK;
}

int pyz_download(void *h_dst, const void *d_src, size_t bytes, void *stream) {
  if (!h_dst || !d_src) return pyz_fail(PYZ_E_INVALID, "null pointer");
  PYZ_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
  PYZ_HIP(hipStreamSynchronize(as_stream(stream)));
  return PYZ_OK;
}

int pyz_wait_flags(const uint64_t *d_flags, int n, uint64_t value, int spin_limit, int *d_fail, void *stream) {
  if (!d_flags) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n < 1 || n > 64) return pyz_fail(PYZ_E_INVALID, "flag count %d outside [1, 64]", n);
  PYZ_LAUNCH(k_wait_flags, dim3(1), dim3(64), 0, as_stream(stream), reinterpret_cast<const unsigned long long *>(d_flags), n,
             (unsigned long long)value, spin_limit, d_fail);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_sync(void *stream) {
  PYZ_HIP(hipStreamSynchronize(as_stream(stream)));
  return PYZ_OK;
}

int pyz_debug_mfma_f64_layout(int32_t *h_out512) {
  if (!h_out512) return pyz_fail(PYZ_E_INVALID, "null pointer");
  int *d = nullptr;
  PYZ_HIP(hipMalloc((void **)&d, 512 * sizeof(int)));
  PYZ_LAUNCH(k_probe_mfma_f64, dim3(1), dim3(64), 0, nullptr, d);
  const hipError_t e = hipMemcpy(h_out512, d, 512 * sizeof(int), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  PYZ_HIP(e);
  return PYZ_OK;
}

int pyz_debug_stamps(uint64_t *h_out, int64_t n_words) {
#ifdef PYZ_STAMPS
  const int64_t total = (int64_t)PYZ_STAMP_KERNELS * PYZ_STAMP_BLOCKS * PYZ_STAMP_WAVES * PYZ_STAMP_SLOTS * 2;
  if (!h_out || n_words < total) return pyz_fail(PYZ_E_INVALID, "need %lld words", (long long)total);
  PYZ_HIP(hipDeviceSynchronize());
  PYZ_HIP(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(pyz_dbg_buf), sizeof(unsigned long long) * total));
  return PYZ_OK;
#else
  (void)h_out;
  (void)n_words;
  return pyz_fail(PYZ_E_INVALID, "not a PYZ_STAMPS build");
#endif
}

// ---------------------------------------------------------------- conv nets: a stem (pyz_conv.h) in front of a Dense tail
int pyz_stem_destroy(pyz_stem *s) {
  if (!s) return PYZ_OK;
  for (int o = 0; o < s->n_ops; ++o) {
    void *ptrs[] = {s->op[o].ktab, s->op[o].out, s->op[o].delta, s->op[o].win};
    for (void *p : ptrs)
      if (p) (void)hipFree(p);
  }
  if (s->part) (void)hipFree(s->part);
  delete s;
  return PYZ_OK;
}

int pyz_stem_create(int in_h, int in_w, int in_c, int n_ops, const int32_t *h_ops, int max_batch, int max_particles,
                    pyz_stem **out) {
  if (!out || !h_ops) return pyz_fail(PYZ_E_INVALID, "null argument");
  *out = nullptr;
  if (n_ops < 1 || n_ops > PYZ_STEM_MAX_OPS) return pyz_fail(PYZ_E_INVALID, "n_ops %d outside [1, %d]", n_ops, PYZ_STEM_MAX_OPS);
  if (in_h < 1 || in_w < 1 || in_c < 1 || in_h > 16384 || in_w > 16384)   // (positions travel as 16-bit pairs in the tap tables)
    return pyz_fail(PYZ_E_INVALID, "input map %d x %d x %d outside [1, 16384] x [1, 16384] x [1, ..)", in_h, in_w, in_c);
  if (max_batch < 1 || max_particles < 1 || max_particles > 65535)
    return pyz_fail(PYZ_E_INVALID, "max_batch must be >= 1 and max_particles in [1, 65535]");
  pyz_stem *s = new pyz_stem();
  s->n_ops = 0;
  s->in_h = in_h; s->in_w = in_w; s->in_c = in_c;
  s->max_batch = max_batch;
  s->max_p = max_particles;
  auto fail = [&](int rc) {
    pyz_stem_destroy(s);
    return rc;
  };
  int H = in_h, W = in_w, C = in_c;
  long long off = 0;
  for (int o = 0; o < n_ops; ++o) {
    const int32_t *d = h_ops + 6 * o;
    StemOp &c = s->op[o];
    c.kind = d[0];
    c.H = H; c.W = W; c.C = C;
    if (c.kind == PYZ_STEM_CONV) {
      c.N = d[1]; c.kh = d[2]; c.kw = d[3]; c.act = d[5];
      if (c.N < 1 || c.kh < 1 || c.kw < 1) return fail(pyz_fail(PYZ_E_INVALID, "op %d: Conv2D filters %d, kernel %d x %d", o, c.N, c.kh, c.kw));
      if (d[4] != 0 && d[4] != 1) return fail(pyz_fail(PYZ_E_INVALID, "op %d: padding %d is neither valid (0) nor same (1)", o, d[4]));
      if (c.act < PYZ_ACT_LINEAR || c.act > PYZ_ACT_SIGMOID) return fail(pyz_fail(PYZ_E_INVALID, "op %d: activation %d is not supported on a Conv2D", o, c.act));
      const int ph = d[4] ? c.kh - 1 : 0, pw = d[4] ? c.kw - 1 : 0;   // TensorFlow's SAME at stride 1: k - 1 in all,
      c.pt = ph / 2;                                                  // the smaller half on top / left
      c.pl = pw / 2;
      if (c.kh > H + ph || c.kw > W + pw)
        return fail(pyz_fail(PYZ_E_SHAPE, "op %d: a %d x %d kernel is larger than the padded %d x %d image", o, c.kh, c.kw, H + ph, W + pw));
      c.OH = H + ph - c.kh + 1;
      c.OW = W + pw - c.kw + 1;
      if ((long long)c.kh * c.kw * C > PYZ_CONV_MAX_K)
        return fail(pyz_fail(PYZ_E_SHAPE, "op %d: %lld taps per filter exceed %d", o, (long long)c.kh * c.kw * C, PYZ_CONV_MAX_K));
      c.K = c.kh * c.kw * C;
      c.KT = (c.K + 2) & ~1;
      c.w_off = off;
      off += (long long)(c.K + 1) * c.N;
    } else if (c.kind == PYZ_STEM_POOL) {
      if (o == 0 || s->op[o - 1].kind != PYZ_STEM_CONV) return fail(pyz_fail(PYZ_E_INVALID, "op %d: a MaxPooling2D must follow a Conv2D", o));
      c.kh = d[1]; c.kw = d[2]; c.N = C;
      if (c.kh < 1 || c.kw < 1) return fail(pyz_fail(PYZ_E_INVALID, "op %d: pool %d x %d", o, c.kh, c.kw));
      if (c.kh > H || c.kw > W) return fail(pyz_fail(PYZ_E_SHAPE, "op %d: a %d x %d pool is larger than its %d x %d input", o, c.kh, c.kw, H, W));
      c.OH = H / c.kh;
      c.OW = W / c.kw;
    } else {
      return fail(pyz_fail(PYZ_E_INVALID, "op %d: unknown kind %d", o, c.kind));
    }
    if ((long long)max_batch * c.OH * c.OW > PYZ_CONV_MAX_ROWS || (long long)max_batch * H * W * C >= (1LL << 31) ||
        (long long)max_batch * c.size() >= (1LL << 31))
      return fail(pyz_fail(PYZ_E_SHAPE, "op %d: max_batch %d x the %d x %d x %d map exceeds the kernels' row or index range", o, max_batch, c.OH, c.OW, c.N));
    H = c.OH; W = c.OW; C = c.N;
    s->n_ops = o + 1;
  }
  if (s->op[0].kind != PYZ_STEM_CONV) return fail(pyz_fail(PYZ_E_INVALID, "the first op must be a Conv2D"));
  s->D = off;
  s->F = (long long)H * W * C;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(pyz_fail(PYZ_E_NODEV, "no HIP device visible"));
  for (int o = 0; o < n_ops; ++o) {
    StemOp &c = s->op[o];
    const size_t bytes = sizeof(float) * (size_t)max_particles * max_batch * c.size() + 64;
    if (hipMalloc((void **)&c.out, bytes) != hipSuccess || hipMalloc((void **)&c.delta, bytes) != hipSuccess)
      return fail(pyz_fail(PYZ_E_OOM, "workspace allocation of %zu bytes failed", bytes));
    s->ws_bytes += 2 * bytes;
    if (c.kind == PYZ_STEM_POOL) {
      if (hipMalloc((void **)&c.win, bytes) != hipSuccess) return fail(pyz_fail(PYZ_E_OOM, "workspace allocation of %zu bytes failed", bytes));
      s->ws_bytes += bytes;
      continue;
    }
    std::vector<int2> tab(c.KT);
    for (int k = 0; k < c.KT; ++k) {
      if (k < c.K) {
        const int cc = k % c.C, j = (k / c.C) % c.kw, i = k / (c.C * c.kw);
        tab[k] = make_int2((i << 16) | j, (i * c.W + j) * c.C + cc);
      } else {
        tab[k] = make_int2(k == c.K ? PYZ_TAP_BIAS : PYZ_TAP_NONE, 0);
      }
    }
    if (hipMalloc((void **)&c.ktab, sizeof(int2) * c.KT) != hipSuccess) return fail(pyz_fail(PYZ_E_OOM, "tap table allocation failed"));
    if (hipMemcpy(c.ktab, tab.data(), sizeof(int2) * c.KT, hipMemcpyHostToDevice) != hipSuccess)
      return fail(pyz_fail(PYZ_E_HIP, "tap table upload failed"));
    s->ws_bytes += sizeof(int2) * c.KT;
  }
  {
    const size_t bytes = stem_part_bytes(s);
    if (hipMalloc((void **)&s->part, bytes) != hipSuccess) return fail(pyz_fail(PYZ_E_OOM, "workspace allocation of %zu bytes failed", bytes));
    s->ws_bytes += bytes;
  }
  *out = s;
  return PYZ_OK;
}

int64_t pyz_stem_param_count(const pyz_stem *s) { return s ? s->D : -1; }
int64_t pyz_stem_feature_count(const pyz_stem *s) { return s ? s->F : -1; }
int64_t pyz_stem_workspace_bytes(const pyz_stem *s) { return s ? (int64_t)s->ws_bytes : -1; }

int pyz_stem_forward(pyz_stem *s, const float *d_theta, int64_t theta_stride, int P, const float *d_x, const int32_t *d_row_idx,
                     int batch, float *d_features, void *stream) {
  int rc = stem_check(s, P, batch);
  if (rc) return rc;
  if (!d_theta || !d_x || !d_features) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (theta_stride < s->D) return pyz_fail(PYZ_E_INVALID, "theta_stride %lld is smaller than the stem's %lld parameters", (long long)theta_stride, s->D);
  hipStream_t st = as_stream(stream);
  stem_forward(s, d_theta, theta_stride, P, d_x, d_row_idx, batch, st);
  const long long n = (long long)batch * s->F;
  PYZ_LAUNCH(k_stem_rows<false>, dim3((unsigned)cdiv(n, 256), P), dim3(256), 0, st, stem_features(s), (long long)s->max_batch * s->F,
             d_features, n, n, (const float *)nullptr, 0LL, 0);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_stem_backward(pyz_stem *s, const float *d_theta, int64_t theta_stride, int P, const float *d_x, const int32_t *d_row_idx,
                      int batch, const float *d_feature_grad, float *d_grad, int64_t grad_stride, void *stream) {
  int rc = stem_check(s, P, batch);
  if (rc) return rc;
  if (!d_theta || !d_x || !d_feature_grad || !d_grad) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (theta_stride < s->D || grad_stride < s->D) return pyz_fail(PYZ_E_INVALID, "a stride is smaller than the stem's %lld parameters", s->D);
  if (!s->forwarded) return pyz_fail(PYZ_E_INVALID, "pyz_stem_backward needs the pyz_stem_forward of the same batch before it");
  hipStream_t st = as_stream(stream);
  const StemOp &last = s->op[s->n_ops - 1];
  const long long n = (long long)batch * s->F, ps = (long long)s->max_batch * s->F;
  PYZ_LAUNCH(k_stem_rows<true>, dim3((unsigned)cdiv(n, 256), P), dim3(256), 0, st, d_feature_grad, n, last.delta, ps, n,
             (const float *)last.out, ps, last.kind == PYZ_STEM_CONV ? last.act : PYZ_ACT_LINEAR);
  stem_backward(s, d_theta, theta_stride, P, d_x, d_row_idx, batch, d_grad, grad_stride, st);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_convnet_forward(pyz_stem *s, pyz_mlp *m, const float *d_theta, int P, const float *d_x, const int32_t *d_row_idx,
                        int batch, float *d_out, void *stream) {
  int rc = convnet_check(s, m, P, batch);
  if (rc) return rc;
  return net_forward(Net{s, m}, d_theta, P, d_x, d_row_idx, batch, d_out, stream);
}

int pyz_convnet_loss_grad(pyz_stem *s, pyz_mlp *m, const float *d_theta, int P, const float *d_x, const void *d_y,
                          const int32_t *d_row_idx, int batch, float *d_grad, float *d_loss, void *stream) {
  int rc = convnet_check(s, m, P, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  hipStream_t st = as_stream(stream);
  if ((rc = set_ctl(m, 0, batch, 0.0f, 0, 0, 0, st))) return rc;
  if ((rc = convnet_loss_backward(s, m, d_theta, P, d_x, d_y, d_row_idx, batch, d_grad, st))) return rc;
  PYZ_LAUNCH(k_loss_finalize, dim3(P), dim3(64), 0, st, m->part, m->cur_nblk, m->ctl, d_loss, m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_convnet_sgd_step(pyz_stem *s, pyz_mlp *m, float *d_theta, const float *d_x, const void *d_y, const int32_t *d_row_idx,
                         int batch, float lr, float *d_loss, void *stream) {
  int rc = convnet_check(s, m, 1, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  const long long Dt = s->D + m->D;
  if ((rc = ensure_bytes((void **)&m->grad, &full(m)->x.grad_cap, sizeof(float) * (size_t)Dt + 64, m))) return rc;
  m->grad_owner = 2;
  hipStream_t st = as_stream(stream);
  if ((rc = set_ctl(m, 0, batch, lr, 0, 0, 0, st))) return rc;
  if ((rc = convnet_loss_backward(s, m, d_theta, 1, d_x, d_y, d_row_idx, batch, m->grad, st))) return rc;
  PYZ_LAUNCH(k_sgd_update, dim3(cdiv(Dt, 256)), dim3(256), 0, st, d_theta, m->grad, Dt, m->ctl, m->part, m->cur_nblk, d_loss,
             m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_convnet_swag_step(pyz_stem *s, pyz_mlp *m, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev_row,
                          const float *d_x, const void *d_y, const int32_t *d_row_idx, int batch, float lr, int64_t n,
                          int update_moments, float *d_loss, void *stream) {
  int rc = convnet_check(s, m, 1, batch);
  if (rc) return rc;
  if ((rc = check_loss_combo(m))) return rc;
  if (!d_theta || !d_mean || !d_sq_mean || !d_x || !d_y || !d_loss) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (n < 0) return pyz_fail(PYZ_E_INVALID, "negative step count");
  const long long Dt = s->D + m->D;
  if ((rc = ensure_bytes((void **)&m->grad, &full(m)->x.grad_cap, sizeof(float) * (size_t)Dt + 64, m))) return rc;
  m->grad_owner = 2;
  hipStream_t st = as_stream(stream);
  if ((rc = set_ctl(m, 0, batch, lr, n, 0, 0, st))) return rc;
  if ((rc = convnet_loss_backward(s, m, d_theta, 1, d_x, d_y, d_row_idx, batch, m->grad, st))) return rc;
  PYZ_LAUNCH(k_swag_update, dim3(cdiv(Dt, 256)), dim3(256), 0, st, d_theta, d_mean, d_sq_mean, d_dev_row, m->grad, Dt,
             update_moments ? 1 : 0, m->ctl, m->part, m->cur_nblk, d_loss, m->nonfinite);
  PYZ_LAUNCH_CHECK();
  return PYZ_OK;
}

int pyz_convnet_predict(pyz_stem *s, pyz_mlp *m, const float *d_weights, int n_samples, const float *d_x, int n,
                        float *d_samples, float *d_mean, float *d_m2, void *stream) {
  if (!s || !m) return pyz_fail(PYZ_E_INVALID, "null plan");
  if (n_samples <= 0 || n <= 0) return pyz_fail(PYZ_E_INVALID, "n_samples and n must be positive");
  int rc = convnet_check(s, m, 1, n);
  if (rc) return rc;
  if (!d_weights || !d_x || !d_mean) return pyz_fail(PYZ_E_INVALID, "null device pointer");
  if (d_m2) return net_predict_moments(Net{s, m}, d_weights, n_samples, d_x, n, d_mean, d_m2, stream);   // (d_samples unused)
  return net_predict(Net{s, m}, d_weights, n_samples, d_x, n, d_samples, d_mean, stream);
}

}  // extern "C"
