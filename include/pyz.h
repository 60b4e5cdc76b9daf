/* pyz.h -- C-ABI of the MI355X (gfx950) backend for the Pyesian.optimizers hot path.
 *
 * The reference (leoelm/Bayesian_inference_for_NN, "Pyesian") has no FFI: the hot
 * path sits behind the Python abstract class `Optimizer`
 * (Pyesian/optimizers/Optimizer.py:14-165) whose subclasses run eager
 * TensorFlow ops.  This header is the boundary a maintainer would bind with
 * ctypes from inside those `step()` methods (INTEGRATION.md shows the stubs).
 * Every entry point cites the reference lines whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C linkage, plain pointers and sizes; no torch / HIP types.
 *   - every function returns int: 0 = PYZ_OK, <0 = error; pyz_last_error()
 *     returns the message of the calling thread's most recent failure.
 *   - pointers named d_* are DEVICE pointers (hipMalloc / torch-ROCm storage)
 *     owned by the caller; h_* are host pointers.  `stream` is a hipStream_t
 *     passed as void* (NULL = the default stream).  Calls enqueue work and
 *     return; scalar outputs live in device memory the caller reads after
 *     synchronising its stream.
 *   - a pyz_mlp handle owns its device workspace and is confined to one host
 *     thread at a time.
 *   - flat parameter order (HMC.py:177-183, SVGD.py:159-160,230-239,
 *     nn/BayesianModel.py:73-77): for each Dense layer, kernel (in x out,
 *     row-major) then bias (out).  "P" below is a particle/chain/sample count:
 *     parameter matrices are (P, D) row-major.
 *   - all arithmetic is float32 (the reference's dtype) unless stated.
 */
#ifndef PYZ_H
#define PYZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYZ_VERSION 302 /* 0.3.2 */

#define PYZ_OK 0
#define PYZ_E_INVALID (-1) /* bad argument / unsupported combination */
#define PYZ_E_SHAPE (-2)   /* batch / particle count exceeds the plan */
#define PYZ_E_HIP (-3)     /* HIP runtime error (message has the HIP string) */
#define PYZ_E_OOM (-4)     /* device allocation failed */
#define PYZ_E_NODEV (-5)   /* no gfx950 device visible */
#define PYZ_E_NAN (-6)     /* pyz_check_finite: a step produced a NaN / Inf loss */

/* activations of a Dense layer (Keras names) */
#define PYZ_ACT_LINEAR 0
#define PYZ_ACT_RELU 1
#define PYZ_ACT_TANH 2
#define PYZ_ACT_SIGMOID 3
#define PYZ_ACT_SOFTMAX 4 /* last layer only */

/* losses produced by Dataset.loss() (Pyesian/datasets/Dataset.py:152-159) */
#define PYZ_LOSS_SCCE 0 /* SparseCategoricalCrossentropy on a softmax last layer; labels int32 (B) */
#define PYZ_LOSS_MSE 1  /* MeanSquaredError; targets float32 (B, out) */
#define PYZ_LOSS_BCE 2  /* BinaryCrossentropy on a last layer of ONE sigmoid unit, from its logit; targets float32 (B, 1) in [0, 1] */

/* SVGD bandwidth: pass this as `gamma` for the median heuristic of SVGD.baseline__kernel (SVGD.py:165-181):
 * h = sqrt(0.5 median(sqdist) / log(M + 1)), K = exp(-sqdist / (2 h^2)), repulsion (-K X + X rowsum K) / h^2,
 * evaluated on the snapshot d_all (PYZ_SWEEP_JACOBI, at most 64 particles, counts in multiples of four). */
#define PYZ_SVGD_GAMMA_MEDIAN (-1.0f)

/* SVGD sweep order */
#define PYZ_SWEEP_GAUSS_SEIDEL 0 /* the reference: particle i sees updated rows 0..i-1 (SVGD.py:100-123) */
#define PYZ_SWEEP_JACOBI 1       /* all rows from one snapshot (multi-GPU mode) */

typedef struct pyz_mlp pyz_mlp;

int pyz_version(void);
const char *pyz_last_error(void);
/* number of visible HIP devices (does not initialise a context beyond the count) */
int pyz_device_count(void);

/* ---- plan -------------------------------------------------------------------
 * Dense stack parsed from the Keras JSON the reference passes to
 * Optimizer.compile (Optimizer.py:43-62).  dims has n_layers+1 entries.
 * max_batch bounds every batch (training, validation, prediction) and
 * max_particles every P passed later; the workspace is sized for both. */
int pyz_mlp_create(int n_layers, const int32_t *h_dims, const int32_t *h_acts, int loss,
                   int max_batch, int max_particles, pyz_mlp **out);
int pyz_mlp_destroy(pyz_mlp *mlp);
int64_t pyz_mlp_param_count(const pyz_mlp *mlp);
int64_t pyz_mlp_workspace_bytes(const pyz_mlp *mlp);

/* ---- G1: Keras Dense forward (called at SGLD.py:55, SGD.py:57, HMC.py:155,
 * BBB.py:144, SVGD.py:106; BayesianModel.py:124).  d_out is (P, batch, out):
 * the model output (softmax applied when the last activation is softmax).
 * d_row_idx (optional, int32[batch]) gathers rows of d_x: row m of the batch
 * is d_x[d_row_idx[m]]. */
int pyz_mlp_forward(pyz_mlp *mlp, const float *d_theta, int n_particles, const float *d_x,
                    const int32_t *d_row_idx, int batch, float *d_out, void *stream);

/* ---- G1-G3: forward + loss + tape.gradient (SGLD.py:54-64, HMC.py:128-136,
 * BBB.py:140-173, SVGD.py:104-111).  d_loss is float32[P] (mean loss over the
 * batch); d_grad is (P, D) or NULL (loss only: the validation passes of
 * BBB.py:203-209 and SVGD.py:126-129). */
int pyz_mlp_loss_grad(pyz_mlp *mlp, const float *d_theta, int n_particles, const float *d_x,
                      const void *d_y, const int32_t *d_row_idx, int batch, float *d_grad,
                      float *d_loss, void *stream);

/* ---- S1: SGD.step update (SGD.py:56-69): theta <- theta - lr * grad. */
int pyz_sgd_step(pyz_mlp *mlp, float *d_theta, const float *d_x, const void *d_y,
                 const int32_t *d_row_idx, int batch, float lr, float *d_loss, void *stream);

/* ---- SWAG.step (Pyesian/optimizers/SWAG.py:43-94; survey 8f rank 2): theta <- theta - lr * grad;
 * when update_moments != 0 (n % frequency == 0): mean / sq_mean running moments with count n and
 * d_dev_row (float32[D], one row of the k x D deviation matrix, may be NULL) <- theta - mean.
 * d_loss receives the batch loss. */
int pyz_swag_step(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev_row,
                  const float *d_x, const void *d_y, const int32_t *d_row_idx, int batch, float lr,
                  int64_t n, int update_moments, float *d_loss, void *stream);

/* ---- ADAM.step (Pyesian/optimizers/ADAM.py:42-84) and the update of VADAM.step (VADAM.py:67-96), one chain.  With g
 * the batch mean of the per-example gradients and s the batch mean of their squares (the reference's squared
 * tape.jacobian, computed here as (A o A)^T (B Delta o B Delta) / B beside A^T Delta, with no Jacobian):
 *   m <- beta_1 m + (1 - beta_1) (g + decay * theta);  v <- beta_2 v + (1 - beta_2) s
 *   theta <- theta - lr * (m / (1 - beta_1^epoch)) / (sqrt(v / (1 - beta_2^epoch)) + denom_eps)
 * ADAM: decay = 0, denom_eps = 1e-3 (ADAM.py:84); VADAM: decay = denom_eps = lam / N (VADAM.py:91,95-96), theta = the
 * perturbed weights.  The bias correction uses the epoch count (>= 1), not the step count, as the reference does.
 * 1 - beta, beta^epoch are evaluated in float64 and rounded to float32 once (the reference's Python-float
 * expressions); beta_1, beta_2 in [0, 1).  d_m / d_v: float32[D]; d_loss receives the batch loss. */
int pyz_adam_step(pyz_mlp *mlp, float *d_theta, float *d_m, float *d_v, const float *d_x, const void *d_y,
                  const int32_t *d_row_idx, int batch, float lr, double beta_1, double beta_2, int64_t epoch,
                  float denom_eps, float decay, float *d_loss, void *stream);

/* ---- VADAM.step's weight perturbation (VADAM.py:59-65): theta += eps / sqrt(num_data (v + lam)), eps ~ N(0,1) from
 * the library's Philox stream (seed, stream 5, step) or from d_eps (float32[D]) when given.  The perturbation is not
 * undone after the step (the reference's weights random-walk). */
int pyz_vadam_perturb(pyz_mlp *mlp, float *d_theta, const float *d_v, float lam, float num_data, int64_t step,
                      uint64_t seed, const float *d_eps, void *stream);

/* ---- BSAM.step (Pyesian/optimizers/BSAM.py:46-119), one chain, both gradient passes of the step on one batch:
 *   perturb (:63-68)      theta += eps * (1 / (N v)), eps ~ N(0,1) from the library's Philox stream (seed, stream 6,
 *                         step) or from d_eps (float32[D]) when given; never undone
 *   first pass (:70-92)   l1, g1 = batch-mean loss and its gradient at the perturbed theta; theta += rho * (g1 / v),
 *                         never undone either; g1 is kept
 *   second pass (:94-117) l2, g2 at the ascended theta, then per element, in this order:
 *       m <- beta_1 m + (1 - beta_1) (g2 + lam * theta);  v <- beta_2 v;
 *       v <- v + (1 - beta_2) (sqrt(v) * |g1 + lam + gam|);  theta <- theta - lr * m / v
 * The square root is taken of the v already scaled by beta_2, the gradient in the v update is the FIRST pass's, lam
 * and gam are added to it as scalars, and the step has neither bias correction nor a square root in its denominator
 * (all as the reference is written).  1 - beta and 1 / N (N = num_data > 0) are evaluated in float64 and rounded to
 * float32 once; beta_1, beta_2 in [0, 1); step >= 0.  d_m / d_v: float32[D] (the reference starts from m = 0, v = 1,
 * :121-141); d_loss: float[2] receives l1, l2.  The ascent and the update run in the epilogues of the two
 * weight-gradient launches when the last layer has at most 32 units, else in two elementwise kernels. */
int pyz_bsam_step(pyz_mlp *mlp, float *d_theta, float *d_m, float *d_v, const float *d_x, const void *d_y,
                  const int32_t *d_row_idx, int batch, float lr, double beta_1, double beta_2, float lam, float rho,
                  float gam, float num_data, int64_t step, uint64_t seed, const float *d_eps, float *d_loss,
                  void *stream);

/* ---- L2/L3: SGLD.step (SGLD.py:54-95).  noise = lr * z, z ~ N(0,1) from the
 * library's Philox stream (seed, step n) or from d_unit_noise (float32[D]) when
 * given; theta += -lr * (grad + noise); mean/sq_mean running moments with
 * count n.  d_loss receives the batch loss. */
int pyz_sgld_step(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, const float *d_x,
                  const void *d_y, const int32_t *d_row_idx, int batch, float lr, int64_t n,
                  uint64_t seed, const float *d_unit_noise, float *d_loss, void *stream);

/* Device-resident multi-step SGLD (the Optimizer.train loop, Optimizer.py:121-134,
 * without per-step host work): step s in [0, n_steps) uses rows
 * d_row_idx[(slot0+s)*max_batch .. +h_batch_sizes[s]) of the resident data set,
 * learning rate h_lr[s] and count n0+s, and writes its batch loss to
 * d_losses[slot0+s].  With use_graph != 0 (and a non-NULL stream) 32 steps are
 * captured once into a hipGraph and replayed; the per-step scalars live in device
 * memory and are advanced by the last kernel of each step. */
int pyz_sgld_run(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, const float *d_x,
                 const void *d_y, const int32_t *d_row_idx, const int32_t *h_batch_sizes,
                 const float *h_lr, int n_steps, int64_t n0, int64_t slot0, uint64_t seed,
                 float *d_losses, int use_graph, void *stream);

/* SGLD, n_chains independent chains in one particle-batched step (an extension: the reference has one chain).
 * d_theta / d_mean / d_sq_mean are float32 (n_chains, D) row-major, d_unit_noise too when given, d_loss float[n_chains].
 * All chains take their gradients on the SAME batch (one particle-batched pass, as pyz_svgd_gradients); chain c then
 * applies pyz_sgld_step's update to row c with z from the Philox stream (seed + c, step n), keyed by the element's index
 * inside the chain: row c draws exactly what a single-chain pyz_sgld_step with seed + c draws.  d_loss[c] = chain c's
 * batch loss.  n_chains must not exceed the plan's max_particles (PYZ_E_SHAPE).  Argument errors (a NULL pointer,
 * n_chains < 1, n < 0, a batch or chain count outside the plan) return before anything touches the GPU. */
int pyz_sgld_chains_step(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, int n_chains,
                         const float *d_x, const void *d_y, const int32_t *d_row_idx, int batch, float lr,
                         int64_t n, uint64_t seed, const float *d_unit_noise, float *d_loss /* [n_chains] */,
                         void *stream);

/* The train loop over pyz_sgld_chains_step without per-step host work: the arguments of pyz_sgld_run; step s uses slot
 * slot0 + s of d_row_idx, h_batch_sizes[s], h_lr[s] and count n0 + s, and writes its n_chains losses to
 * d_losses[(slot0 + s) * n_chains ..].  The per-step scalars live in device memory and are advanced by the last kernel
 * of each step; nothing synchronises inside the call.  The steps are enqueued one after the other, each launched for its
 * own batch size (no hipGraph, whatever use_graph says: pyz_last_run_info reports them as eager steps).  Results equal
 * n_steps calls of pyz_sgld_chains_step bit for bit, on ragged batches and across epoch changes. */
int pyz_sgld_chains_run(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, int n_chains,
                        const float *d_x, const void *d_y, const int32_t *d_row_idx,
                        const int32_t *h_batch_sizes, const float *h_lr, int n_steps, int64_t n0, int64_t slot0,
                        uint64_t seed, float *d_losses /* (slots, n_chains) */, int use_graph, void *stream);

/* ---- SGLD lanes: n_lanes chains that differ by their hyper-parameters (a grid search's points side by side).
 * pyz_sgld_chains_step with a learning rate per lane, h_lr[c] (HOST floats: they ride in the launch), and the Philox seed
 * seed + c * seed_stride: seed_stride = 1 is the chains step (equal rates: bit for bit), seed_stride = 0 gives every lane
 * ONE noise stream, so that lanes with equal starts differ by their rates alone.  d_unit_noise (n_lanes, D) or NULL.
 * PYZ_E_INVALID, with no device touched: a null plan, a null pointer among the required ones, n_lanes < 1, a negative
 * count, seed_stride outside {0, 1}.  PYZ_E_SHAPE: n_lanes above the plan's max_particles or above PYZ_MAX_LANES. */
#define PYZ_MAX_LANES 64
int pyz_sgld_lanes_step(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, int n_lanes, const float *d_x,
                        const void *d_y, const int32_t *d_row_idx, int batch, const float *h_lr /* host, [n_lanes] */,
                        int64_t n, uint64_t seed, int seed_stride, const float *d_unit_noise,
                        float *d_loss /* [n_lanes] */, void *stream);

/* pyz_sgld_chains_run over pyz_sgld_lanes_step: step s takes the rates h_lr[s * n_lanes ..] (host, (n_steps, n_lanes)
 * row-major).  Every step is enqueued for its own batch size (no hipGraph: pyz_last_run_info reports eager steps), nothing
 * synchronises inside the call, and the results equal n_steps calls of pyz_sgld_lanes_step bit for bit. */
int pyz_sgld_lanes_run(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, int n_lanes, const float *d_x,
                       const void *d_y, const int32_t *d_row_idx, const int32_t *h_batch_sizes,
                       const float *h_lr /* host, (n_steps, n_lanes) */, int n_steps, int64_t n0, int64_t slot0,
                       uint64_t seed, int seed_stride, float *d_losses /* (slots, n_lanes) */, void *stream);

/* The score of every lane on n contiguous rows of d_x / d_y (d_y as for pyz_mlp_loss_grad): d_loss_sum[c] = the sum over the
 * rows of the plan's per-row loss (the loss head's float32 expressions; summed in float64, one partial per workgroup, the
 * partials added in workgroup order: the same call gives the same bits), d_errors[c] (may be NULL) = the rows whose first
 * argmax differs from the label (SCCE), the rows with (p > 0.5) != (y > 0.5) (BCE), 0 (MSE).  d_weights (n_lanes, D); more
 * lanes than max_particles go through in chunks.  n <= max_batch (PYZ_E_SHAPE); rows at or beyond n are never read. */
int pyz_lane_scores(pyz_mlp *mlp, const float *d_weights, int n_lanes, const float *d_x, const void *d_y, int n,
                    double *d_loss_sum /* [n_lanes] */, int64_t *d_errors /* [n_lanes] or NULL */, void *stream);

/* Device-resident multi-step SGD (SGD.py:42-69 under the train loop of Optimizer.py:121-134): the
 * arguments of pyz_sgld_run without the moment vectors, count and seed; step s applies
 * theta <- theta - h_lr[s] * grad on its batch and writes the batch loss to d_losses[slot0+s].
 * Needs the fused step (last layer of at most 32 units). */
int pyz_sgd_run(pyz_mlp *mlp, float *d_theta, const float *d_x, const void *d_y,
                const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr,
                int n_steps, int64_t slot0, float *d_losses, int use_graph, void *stream);

/* Device-resident multi-step SWAG (SWAG.py:43-94 under the train loop): step s has count n0 + s; when the
 * count is a multiple of `frequency` the moments are updated and theta - mean goes to row
 * min(ceil(count / frequency), k - 1) of d_dev (float32 (k, D), row = one column of the reference's
 * deviation matrix).  The bookkeeping assumes the chain started at count 0 with every step run through
 * pyz_swag_step / pyz_swag_run.  Needs the fused step. */
int pyz_swag_run(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev, int k,
                 int frequency, const float *d_x, const void *d_y, const int32_t *d_row_idx,
                 const int32_t *h_batch_sizes, const float *h_lr, int n_steps, int64_t n0,
                 int64_t slot0, float *d_losses, int use_graph, void *stream);

/* ---- SGD / SWAG members: n_members models trained in one particle-batched step (an extension: the reference trains
 * one; P of them are a deep ensemble, or the components of a MultiSWAG mixture).  The state is float32 (n_members, D)
 * row-major; all members take their gradients on the SAME batch (one particle-batched pass, as pyz_sgld_chains_step),
 * then member c's row takes the single-model update.  d_loss[c] / d_losses[(slot0 + s) * n_members + c] = member c's
 * batch loss.  PYZ_E_INVALID, with no device touched: a null plan, a null pointer among the required ones,
 * n_members < 1, k < 1, frequency < 1, a negative count.  PYZ_E_SHAPE: n_members above the plan's max_particles, a
 * batch outside the plan.  The runs enqueue every step for its own batch size (no hipGraph, whatever use_graph says:
 * pyz_last_run_info reports eager steps), nothing synchronises inside the call, and the results equal n_steps calls of
 * the step bit for bit, on ragged batches and across epoch changes.
 *
 * pyz_sgd_members_step (SGD.py:42-84): theta <- theta - lr grad per member; with update_mean != 0 (the caller's
 * n % frequency == 0) row c of d_mean receives member c's new weights, else d_mean is neither read nor written. */
int pyz_sgd_members_step(pyz_mlp *mlp, float *d_theta, float *d_mean, int n_members, const float *d_x,
                         const void *d_y, const int32_t *d_row_idx, int batch, float lr, int64_t n, int update_mean,
                         float *d_loss /* [n_members] */, void *stream);

/* The train loop over pyz_sgd_members_step (SGD.py:42-84 inside Optimizer.py:121-134): step s has count n0 + s and
 * copies the weights to d_mean when that count is a multiple of `frequency` -- decided on the device, so the run is
 * not cut there as the single-model caller of pyz_sgd_run cuts it. */
int pyz_sgd_members_run(pyz_mlp *mlp, float *d_theta, float *d_mean, int n_members, int frequency, const float *d_x,
                        const void *d_y, const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr,
                        int n_steps, int64_t n0, int64_t slot0, float *d_losses /* (slots, n_members) */,
                        int use_graph, void *stream);

/* pyz_swag_members_step (SWAG.py:61-92): pyz_swag_step's update per member, in its float32 expressions.  d_dev is
 * float32 (n_members, k, D): member c's k deviation rows, each one column of the reference's deviation matrix.  With
 * update_moments != 0 the moments move and theta - mean goes to row dev_col of every member's block; dev_col < 0
 * writes no row (pyz_swag_step's d_dev_row = NULL), dev_col >= k is PYZ_E_INVALID.  Without update_moments the
 * moments and deviations are neither read nor written. */
int pyz_swag_members_step(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev, int k,
                          int n_members, const float *d_x, const void *d_y, const int32_t *d_row_idx, int batch,
                          float lr, int64_t n, int update_moments, int dev_col, float *d_loss /* [n_members] */,
                          void *stream);

/* The train loop over pyz_swag_members_step (SWAG.py:43-94 inside Optimizer.py:121-134): the bookkeeping of
 * pyz_swag_run per member -- moments on the counts that are multiples of `frequency`, the deviation into row
 * min(ceil(count / frequency), k - 1) -- which assumes the members started at count 0 with every step run: n0 < slot0
 * is PYZ_E_INVALID. */
int pyz_swag_members_run(pyz_mlp *mlp, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev, int k,
                         int frequency, int n_members, const float *d_x, const void *d_y, const int32_t *d_row_idx,
                         const int32_t *h_batch_sizes, const float *h_lr, int n_steps, int64_t n0, int64_t slot0,
                         float *d_losses /* (slots, n_members) */, int use_graph, void *stream);

/* What the last pyz_sgld_run / pyz_sgd_run / pyz_swag_run call on this plan did: steps that ran inside replayed
 * hipGraphs, steps launched eagerly, and the number of graph launches.  With use_graph != 0 on a non-NULL
 * stream a run of any length is replayed from graphs: chunks of 32 steps (PYZ_GRAPH_STEPS) and one graph for
 * the remainder, captured for its exact length and kept (seven lengths, least recently used one replaced). */
int pyz_last_run_info(const pyz_mlp *mlp, int32_t *h_graph_steps, int32_t *h_eager_steps,
                      int32_t *h_graph_launches);

/* *h_captures = the graphs the last pyz_sgd_run / pyz_swag_run / pyz_sgld_run / pyz_bbb_run call on this plan had to
 * capture (0: every chunk was replayed from the cache, or launched eagerly).  The cache holds the graphs of one set of
 * arguments (the caller's pointers, the seed, the largest batch, the hyper-parameters baked into the launches); a call
 * with another set, or one behind a call that made the plan move one of its lazily grown buffers (more particles than
 * any call before it), captures again. */
int pyz_sgld_run_info(const pyz_mlp *mlp, int32_t *h_captures);

/* *h_form = where the steps of the last device-resident run on this plan (pyz_sgd_run / pyz_swag_run / pyz_sgld_run /
 * pyz_bbb_run / pyz_adam_run / pyz_bsam_run) found their batch rows: 0 = each step gathered its own, 1 = assembled one
 * step ahead as contiguous rows, 2 = assembled one step ahead as the two fragment-major images of DESIGN section 3
 * (PYZ_BATCH_FRAG, input width a multiple of 8; the SGD / SWAG / SGLD / BBB runs only).  Results do not depend on it. */
int pyz_run_batch_form(const pyz_mlp *mlp, int32_t *h_form);

/* Non-finite sentinel (the reference prints the loss every step, Optimizer.py:123, so a diverged chain is
 * seen at once; here losses stay on the device): every kernel that finalises a step's loss counts NaN / Inf
 * results.  Synchronises `stream`, returns PYZ_E_NAN if any step since the last call was non-finite (the
 * count is in the message) and resets the count. */
int pyz_check_finite(pyz_mlp *mlp, void *stream);

/* Measurement (bench.py roofline leg): between pyz_probe_begin and pyz_probe_end every kernel the calling
 * thread launches through this library carries a start / stop event pair of its own (hipExtLaunchKernelGGL:
 * the dispatch's begin / end timestamps, i.e. the duration rocprofv3 --kernel-trace reports; no packet is
 * added between the kernels of a pipeline).  While a probe is open the *_run entry points launch eagerly.
 * pyz_probe_end synchronises `stream` and returns, in launch order, each launch's duration in microseconds
 * (h_us[max_launches]) and the kernel expression of its launch site (h_names: max_launches rows of
 * name_stride bytes, NUL terminated; may be NULL); *h_n = launches recorded. */
int pyz_probe_begin(int max_launches);
int pyz_probe_end(void *stream, float *h_us, char *h_names, int name_stride, int *h_n);

/* ---- B2-B4: BBB.step (BBB.py:128-201).  d_mu / d_rho are the variational
 * parameters (D each); eps ~ N(0,1) from Philox (seed, step) or d_eps.
 * Writes the sampled weights to d_w (D, used by the validation pass), the
 * cost (loss + alpha * (log q - log p)) to d_cost[0] and the data loss to
 * d_cost[1].  prior_rho is the raw rho: sigma_p = softplus(prior_rho).  A list-valued
 * GaussianPrior (GaussianPrior.py:50-69) is passed as the optional per-element vectors
 * d_prior_mean_vec / d_prior_rho_vec (float32[D]; NULL = the scalars). */
int pyz_bbb_step(pyz_mlp *mlp, float *d_mu, float *d_rho, float *d_w, const float *d_x,
                 const void *d_y, const int32_t *d_row_idx, int batch, float lr, float alpha,
                 float prior_mean, float prior_rho, const float *d_prior_mean_vec,
                 const float *d_prior_rho_vec, int64_t step, uint64_t seed,
                 const float *d_eps, float *d_cost, void *stream);

/* The BBB train loop (BBB.step inside Optimizer.train, Optimizer.py:121-134) as ONE device-resident run of n_steps
 * steps, replayed from captured hipGraphs like pyz_sgld_run: d_row_idx (slots, max_batch) / h_batch_sizes / h_lr as
 * there; step i of the call is optimizer step step0 + i (its Philox step) and writes {cost, data loss, log q - log p}
 * to d_costs[4 (slot0 + i) ..].  Needs a last layer of at most 32 units.  val_plan (optional; a second plan of the same
 * model with max_batch >= n_val): on the steps BBB.py:203 validates (step % 10 != 0) the validation split d_val_x /
 * d_val_y is forwarded through the weights the step sampled and its mean loss goes to d_val_losses[slot0 + i].
 * Results equal n_steps calls of pyz_bbb_step (+ pyz_mlp_loss_grad on the validation plan) bit for bit. */
int pyz_bbb_run(pyz_mlp *mlp, float *d_mu, float *d_rho, float *d_w, const float *d_x, const void *d_y,
                const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr, int n_steps,
                float alpha, float prior_mean, float prior_rho, const float *d_prior_mean_vec,
                const float *d_prior_rho_vec, int64_t step0, int64_t slot0, uint64_t seed, float *d_costs,
                pyz_mlp *val_plan, const float *d_val_x, const void *d_val_y, int n_val,
                float *d_val_losses, int use_graph, void *stream);

/* ---- BBB lanes: n_lanes Bayes-by-Backprop posteriors that differ by their hyper-parameters (the points of a grid search
 * side by side).  pyz_bbb_step for the n_lanes rows of d_mu / d_rho / d_w (n_lanes, D) on ONE shared batch: lane c steps
 * with h_lr[c] and h_alpha[c] against the scalar prior (h_prior_mean[c], softplus(h_prior_rho[c])) -- HOST floats, [n_lanes]
 * each: they ride in the launch -- or against the per-element vectors d_prior_mean_vec / d_prior_rho_vec (D, shared by
 * the lanes; both or neither), and draws eps from the Philox seed seed + c * seed_stride (seed_stride = 0: ONE stream for
 * every lane, 1: the stream of a single pyz_bbb_step with seed + c) or takes row c of d_eps (n_lanes, D).  Lane c's
 * {cost, data loss, log q - log p, 0} go to d_cost[4 c ..].  A lane's sampled weights and its log q - log p are the bits
 * pyz_bbb_step gives from the same mu, rho, eps and prior; the same call gives the same bits.
 * PYZ_E_INVALID, with no device touched: a null plan, a null pointer among the required ones, n_lanes < 1, a negative
 * step, seed_stride outside {0, 1}, exactly one of the two prior vectors.  PYZ_E_SHAPE: n_lanes above the plan's
 * max_particles or above PYZ_MAX_LANES. */
int pyz_bbb_lanes_step(pyz_mlp *mlp, float *d_mu, float *d_rho, float *d_w, int n_lanes, const float *d_x, const void *d_y,
                       const int32_t *d_row_idx, int batch, const float *h_lr, const float *h_alpha,
                       const float *h_prior_mean, const float *h_prior_rho /* host, [n_lanes] each */,
                       const float *d_prior_mean_vec, const float *d_prior_rho_vec /* (D) shared, or NULL */,
                       int64_t step, uint64_t seed, int seed_stride, const float *d_eps /* (n_lanes, D) or NULL */,
                       float *d_cost /* (n_lanes, 4) */, void *stream);

/* n_steps steps of pyz_bbb_lanes_step without host work in between: d_row_idx (slots, max_batch) / h_batch_sizes as for
 * pyz_sgld_run, the lanes' four host tables hold for every step of the call, step i is optimizer step step0 + i (its
 * Philox step) and writes its (n_lanes, 4) costs to row slot0 + i of d_costs.  Every step is enqueued for its own batch
 * size (no hipGraph: pyz_last_run_info reports eager steps), nothing synchronises inside the call, there is no validation
 * forward, and the results equal n_steps calls of pyz_bbb_lanes_step bit for bit. */
int pyz_bbb_lanes_run(pyz_mlp *mlp, float *d_mu, float *d_rho, float *d_w, int n_lanes, const float *d_x, const void *d_y,
                      const float *h_lr, const float *h_alpha, const float *h_prior_mean,
                      const float *h_prior_rho /* host, [n_lanes] each */, const float *d_prior_mean_vec,
                      const float *d_prior_rho_vec /* (D) shared, or NULL */, const int32_t *d_row_idx,
                      const int32_t *h_batch_sizes, int n_steps, int64_t step0, int64_t slot0, uint64_t seed,
                      int seed_stride, float *d_costs /* (slots, n_lanes, 4) */, void *stream);

/* The ADAM / VADAM train loop (ADAM.step / VADAM.step inside Optimizer.train, ADAM.py:42-86, VADAM.py:45-99,
 * Optimizer.py:121-134) as ONE device-resident run of n_steps steps, replayed from captured hipGraphs like pyz_sgld_run:
 * d_row_idx (slots, max_batch) / h_batch_sizes / h_lr / slot0 as there.  h_epochs[s] (>= 1) is the epoch count step s uses
 * for its bias correction (the host knows where epochs begin); 1 - beta^epoch is evaluated per step as pyz_adam_step does
 * (float64, rounded to float32 once) and kept in a device table beside the learning rates.  Step i of the call is
 * optimizer step step0 + i and writes its batch loss to d_losses[slot0 + i].  perturb != 0 selects VADAM: the perturbation
 * of pyz_vadam_perturb (Philox stream 5, step step0 + i, no injected noise; lam, num_data > 0) runs before each step's
 * gradients -- for the first step of the call as a launch, for every later one in the epilogue of the weight-gradient
 * kernel of the step before it, which holds the v and the weight it reads (PYZ_ADAM_FUSE_PERTURB=0, read once: a launch
 * per step).  The last step of a call leaves the weights unperturbed.  Every step is launched for its own batch size, so
 * a graph holds steps of one batch size (chunks of PYZ_GRAPH_STEPS inside a stretch of equal batches, one graph for the
 * stretch's remainder; 32 graphs by length, batch size and starting slot, least recently used one replaced).
 * Needs the fused step (last layer of at most 32 units), else PYZ_E_INVALID; every refusal returns before anything is
 * enqueued.  d_theta, d_m, d_v and every loss equal n_steps calls of pyz_adam_step (with pyz_vadam_perturb before each
 * when perturb) bit for bit, on ragged batches and across epoch changes, with use_graph on or off.  pyz_last_run_info
 * reports the split; while a probe is open the run launches eagerly. */
int pyz_adam_run(pyz_mlp *mlp, float *d_theta, float *d_m, float *d_v, const float *d_x, const void *d_y,
                 const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr,
                 const int64_t *h_epochs, int n_steps, double beta_1, double beta_2, float denom_eps,
                 float decay, int perturb, float lam, float num_data, int64_t step0, int64_t slot0,
                 uint64_t seed, float *d_losses, int use_graph, void *stream);

/* The BSAM train loop (BSAM.step inside Optimizer.train, BSAM.py:46-119, Optimizer.py:121-134) as ONE device-resident
 * run, as pyz_adam_run: step i of the call is optimizer step step0 + i (its Philox step, stream 6) and writes {l1, l2} to
 * d_losses[2 (slot0 + i) ..].  Both passes of a step run on one StepCtl slot; the second pass's weight-gradient kernel
 * advances it and -- unless PYZ_ADAM_FUSE_PERTURB=0 -- stores the weights with the perturbation of step i + 1 applied.
 * Results equal n_steps calls of pyz_bsam_step bit for bit. */
int pyz_bsam_run(pyz_mlp *mlp, float *d_theta, float *d_m, float *d_v, const float *d_x, const void *d_y,
                 const int32_t *d_row_idx, const int32_t *h_batch_sizes, const float *h_lr, int n_steps,
                 double beta_1, double beta_2, float lam, float rho, float gam, float num_data,
                 int64_t step0, int64_t slot0, uint64_t seed, float *d_losses, int use_graph, void *stream);

/* *h_captures = the graphs the last pyz_adam_run / pyz_bsam_run on the plan had to capture (0: every stretch was
 * replayed from the cache). */
int pyz_adam_run_info(const pyz_mlp *mlp, int32_t *h_captures);

/* ---- H2-H5: one HMC proposal (HMC.py:74-104) for P independent chains on the
 * full training split (d_x, d_y, n_rows).  d_q (P, D) is updated in place when
 * accepted.  Momentum p = m * z with z from Philox (seed, step, chain) or
 * d_unit_p (P, D).  h_uniform[P] are the host uniforms of random.random();
 * burning != 0 forces acceptance.  Outputs (device, float32): d_stats (P, 8) =
 * {accepted, loss, U0, K0, U1, K1, log_ratio, 0}.  prior_sigma is the raw rho
 * (negative => NaN potential, every non-burn proposal rejected, HMC.py:149-159).
 * d_prior_mean_vec / d_prior_sigma_vec: optional per-element prior (float32[D], shared by the
 * chains) for list-valued priors; NULL = the scalars.
 * Small 2-layer models (inputs, classes <= 8, hidden + classes <= 64) run with the chain state in LDS:
 * one workgroup per chain for many chains, or -- for at most 16 chains and >= 192 rows -- row slices
 * spread over up to 32 workgroups per chain with one launch per gradient evaluation, replayed as a
 * hipGraph when `stream` is not the default stream.  Results do not depend on the path beyond float32
 * summation order. */
int pyz_hmc_step(pyz_mlp *mlp, float *d_q, int n_chains, const float *d_x, const void *d_y,
                 int n_rows, int L, float epsilon, float m, float prior_mean, float prior_sigma,
                 const float *d_prior_mean_vec, const float *d_prior_sigma_vec,
                 int burning, const float *h_uniform, int64_t step, uint64_t seed,
                 const float *d_unit_p, float *d_stats, void *stream);

/* The quiet HMC.train (HMC.py:106-125) as ONE device-resident run: n_steps consecutive proposals of pyz_hmc_step
 * (same model, data, L, epsilon, m and prior; momentum from Philox) with no host work in between.  h_uniform
 * (host, float32 [n_steps x n_chains], proposal-major: the random.random() draws in the reference's order) is
 * uploaded once; proposal i of the call uses Philox step step0 + i, runs with burning = 1 and records nothing while
 * i < n_burn, and writes its eight statistics (the layout of pyz_hmc_step's d_stats, stats[7] = -1 on a give-up) to
 * d_stats_all[(slot0 + i) * n_chains * 8 ..].  The sample record of HMC.py:92-103 is kept on the device: d_samples
 * float32 (n_chains, cap, D), d_freq int32 (n_chains, cap), d_count int32 [n_chains] (zero for a fresh record; a
 * later call goes on where the counts stand).  After a non-burning proposal an accepted chain c gets
 * d_samples[c][count] = q[c], d_freq[c][count] = 1, count += 1, a rejected one d_freq[c][count - 1] += 1; a chain
 * with count == 0 first records its starting q with frequency 1 (HMC.py:75-77); a proposal that gave up records
 * nothing; a chain out of rows records nothing and counts in d_fail, never writing past cap rows.  d_fail int32 [4]
 * (the caller zeroes it; counts add up over calls) = {accepted proposals that found no row, proposals (per chain)
 * that gave up, non-finite losses, proposals done}.  With use_graph != 0 on a non-NULL stream the sliced forms
 * (at most 16 chains, >= 192 rows) replay hipGraphs of 16 proposals (PYZ_HMC_RUN_CHUNK) and one of the exact
 * remaining length, captured once per length and kept; the one-workgroup form and the generic sequence are launched
 * eagerly, still without a synchronisation; the first proposal of a call is always eager.  pyz_last_run_info
 * reports the split of the last call, pyz_hmc_run_info the graphs it had to capture.  Argument errors (a NULL
 * pointer, n_steps <= 0, n_burn outside [0, n_steps], cap < 1, negative step0 / slot0) return PYZ_E_INVALID before
 * anything touches the GPU.  q, every proposal's statistics and the accept sequence equal n_steps calls of
 * pyz_hmc_step bit for bit.  A non-finite loss of a proposal also counts in the plan's sentinel (pyz_check_finite; the
 * generic sequence counts there per gradient evaluation as well); give-ups and chains out of rows are reported in
 * d_fail only.  As with every entry point, one host thread drives a plan at a time: the run calls pyz_hmc_step's dispatch
 * on the plan, which must not be entered from another thread meanwhile.  pyz_hmc_run_info: *h_captures = the graphs the
 * last pyz_hmc_run on the plan had to capture (0: every chunk was replayed from the cache). */
int pyz_hmc_run(pyz_mlp *mlp, float *d_q, int n_chains, const float *d_x, const void *d_y, int n_rows, int L,
                float epsilon, float m, float prior_mean, float prior_sigma, const float *d_prior_mean_vec,
                const float *d_prior_sigma_vec, const float *h_uniform, int n_steps, int n_burn, int64_t step0,
                int64_t slot0, uint64_t seed, float *d_stats_all, float *d_samples, int32_t *d_freq,
                int32_t *d_count, int cap, int32_t *d_fail, int use_graph, void *stream);
int pyz_hmc_run_info(const pyz_mlp *mlp, int32_t *h_captures);

/* ---- V2-V4: SVGD.step (SVGD.py:84-141).  d_particles (P_local, D) float32 are
 * this rank's rows [row0, row0+P_local) of the (M, D) particle matrix; d_all
 * (M, D) is the matrix the kernel row is evaluated against (== d_particles under
 * PYZ_SWEEP_GAUSS_SEIDEL; under PYZ_SWEEP_JACOBI a SEPARATE snapshot -- the all-gathered
 * matrix, or on one GPU a copy or the other of two alternating buffers: every row is
 * read from it while d_particles is written, so a d_particles that overlaps
 * [d_all, d_all + M D) is refused with PYZ_E_INVALID before anything is enqueued).  d_adam_m/v are
 * the Keras-legacy-Adam slots (P_local, D); t is the 1-based Adam step.  The
 * squared distances, the RBF kernel and the repulsion sum are evaluated in float64.  gamma > 0 is
 * the fixed bandwidth (reference: 1.0); PYZ_SVGD_GAMMA_MEDIAN selects the median heuristic.  d_loss[0] = sum_i loss_i / M over the
 * local rows.  Under PYZ_SWEEP_JACOBI with M <= 64 and local rows in multiples of four (row0 too) the
 * sweep reads the particle matrix once per pass for all rows (squared distances through the Gram matrix on the
 * float64 matrix cores); a shard then gets the rows of the whole-matrix call.  Under PYZ_SWEEP_GAUSS_SEIDEL with M <= 64 and D <= 196 608 the sweep is one launch
 * per particle that reads the matrix once; otherwise two launches per particle.  The paths agree within
 * float32 rounding of phi. */
int pyz_svgd_step(pyz_mlp *mlp, float *d_particles, int n_local, const float *d_all, int n_total,
                  int row0, float *d_adam_m, float *d_adam_v, const float *d_x, const void *d_y,
                  const int32_t *d_row_idx, int batch, float lr, float gamma, int64_t t, int sweep,
                  float *d_loss, void *stream);

/* The two phases of pyz_svgd_step as calls of their own, for callers that overlap the exchange of the particle
 * matrix (the RCCL all-gather of the Jacobi sweep) with phase 1: pyz_svgd_gradients computes the loss gradients
 * of the local particles (SVGD.py:104-111; they stay inside the plan) and needs no other rank's rows;
 * pyz_svgd_sweep does the rest (kernel rows, repulsion, Adam, d_loss) and is the first reader of d_all. */
int pyz_svgd_gradients(pyz_mlp *mlp, const float *d_particles, int n_local, const float *d_x, const void *d_y,
                       const int32_t *d_row_idx, int batch, void *stream);
int pyz_svgd_sweep(pyz_mlp *mlp, float *d_particles, int n_local, const float *d_all, int n_total, int row0,
                   float *d_adam_m, float *d_adam_v, float lr, float gamma, int64_t t, int sweep, float *d_loss,
                   void *stream);

/* pyz_svgd_sweep under PYZ_SWEEP_JACOBI (at most 64 particles, row0 and n_local multiples of four) in its two halves,
 * for callers that place work -- or a collective of their own -- between them (SVGD.py:54-68,183-202 is a function of
 * the particle matrix alone; SVGD.py:112-123 needs the gradients too):
 *   pyz_svgd_kernel_matrix  squared distances of rows [row0, row0 + n_local) of the snapshot d_all (M, D) against all
 *                           of it (float64), the bandwidth when gamma == PYZ_SVGD_GAMMA_MEDIAN, K rows and their sums;
 *                           they stay inside the plan.  It touches neither the gradients nor the losses of phase 1:
 *                           it may run on ANOTHER stream than pyz_svgd_gradients, at the same time;
 *   pyz_svgd_combine        phi, the legacy Adam step of every local row, d_loss -- ordered by the caller after BOTH
 *                           (stream order or events); same d_all, rows and gamma as the kernel-matrix call.
 * kernel_matrix + combine on one stream is what pyz_svgd_sweep runs for such shapes (bit-identical results).
 * Under PYZ_SWEEP_JACOBI d_particles is only WRITTEN (the rows' current values are read from rows [row0, ...) of
 * d_all -- by pyz_svgd_step's gradient pass too): a one-GPU caller may alternate two (M, D) buffers instead of copying
 * the matrix every step.  (pyz_svgd_gradients takes the current rows explicitly.)
 * PYZ_E_INVALID for shapes the all-rows-at-once kernels do not take (use pyz_svgd_sweep), and from pyz_svgd_combine /
 * pyz_svgd_sweep when the plan does not hold what they consume (another entry point used its buffers in between).
 * A plan serves one stream at a time, with this one exception. */
int pyz_svgd_kernel_matrix(pyz_mlp *mlp, const float *d_all, int n_total, int row0, int n_local, float gamma,
                           void *stream);
int pyz_svgd_combine(pyz_mlp *mlp, float *d_particles, int n_local, const float *d_all, int n_total, int row0,
                     float *d_adam_m, float *d_adam_v, float lr, float gamma, int64_t t, float *d_loss,
                     void *stream);

/* The distance pass of pyz_svgd_kernel_matrix split over the ELEMENTS of the particles, for sharded runs (each
 * rank reads D / world of the gathered matrix instead of all of it; the exchange is PYZ_SVGD_GROUPS x 32 KB, the caller's):
 * the blocks of the pass form PYZ_SVGD_GROUPS groups of consecutive blocks;
 *   pyz_svgd_gram_groups           partial squared distances of ALL pairs over groups [g_lo, g_hi) of d_all (M, D), M a multiple
 *                                  of four <= 64, summed per group into d_groups[(g * 64 + i) * 64 + j] (float64; entries of
 *                                  other groups are not touched) -- rank r of a world that divides 8 takes groups
 *                                  [8 r / world, 8 (r + 1) / world) and all-gathers its slice;
 *   pyz_svgd_kernel_matrix_groups  pyz_svgd_kernel_matrix with the complete d_groups (PYZ_SVGD_GROUPS, 64, 64) in place of the
 *                                  pass over d_all (still named: pyz_svgd_combine checks it).
 * pyz_svgd_kernel_matrix sums its own partials in the same order (groups, then a fixed tree over the groups), so both
 * routes give the same bits for any split of the groups over ranks (SVGD.py:183-202 per pair, float64). */
#define PYZ_SVGD_GROUPS 8
int pyz_svgd_gram_groups(pyz_mlp *mlp, const float *d_all, int n_total, int g_lo, int g_hi, double *d_groups, void *stream);
int pyz_svgd_kernel_matrix_groups(pyz_mlp *mlp, const double *d_groups, const float *d_all, int n_total, int row0,
                                  int n_local, float gamma, void *stream);

/* ---- F1: FSVI.step (Pyesian/optimizers/FSVI.py:60-147; Rudner et al., "Tractable Function-Space Variational Inference in
 * Bayesian Neural Networks"), as DESIGN assumption A8 defines it.  State: d_mu float32[D] with one Keras-legacy-Adam slot pair
 * d_adam_m / d_adam_v (only optimizers[0] is used, :136), the k particles d_particles (k, D), the 1-based step t.
 * With b = batch rows of this step (d_row_idx, or rows 0 .. b - 1 of d_x), B = batch_size, n = b + B, F inputs:
 *   Xp_i (n, F): the batch rows + z_i, then X_M + (z_0 + ... + z_i), a sequential float32 sum (:86-89, 106), with
 *     X_M[r][c] = lo[c] + u (hi[c] - lo[c]) (:197-212) and z_i = 0.1 N(0, 1) (:87);
 *   f_i = model(W_i; Xp_i); ll_i = mean over the batch rows of (f_i - y)^2, its gradient scaled by k / B (:95-98);
 *   alpha_i = (K_i + 1e-6 I)^-1 f_i with K_i[r][s] = exp(-|Xp_i[r] - Xp_i[s]|^2 / 2), float64 throughout (:149-165);
 *   c2_i = -(K_w + 1e-3 I)^-1 rhs over the D weights of W_i as scalar points, float64, rounded once (:177-195);
 *   g = sum_i [(k / B) grad ll_i - (1 / k) J_i^T alpha_i - (1 / k) c2_i], one backward pass per particle, fixed-order sums (:115-136);
 *   Adam (beta_1 0.9, beta_2 0.999, epsilon 1e-7, step t) on d_mu, then W_i = mu + eps_i for every particle (:135-138, 228-231).
 * d_loss[0] = sum_i ll_i / k (:123, 147).  Draws: Philox stream PYZ_STREAM_FSVI = 9 (csrc/pyz_rng.h) of `seed`, step 4 t for
 * the uniforms of X_M (element r F + c), 4 t + 1 for the normals of z (element i F + c), 4 t + 2 for eps (element i D + e);
 * or the caller's: d_xm (B, F), d_noise (k, F) (the z_i themselves), d_eps (k, D); NULL selects the stream.  d_lo / d_hi
 * float32[F] are needed without d_xm.  Optional outputs (NULL: not written): d_alpha (k, n) float64, d_stein (k, D) the c2_i,
 * d_grad float32[D] g, d_xp (k, n, F), d_f (k, n) the f_i.
 * PYZ_E_INVALID, before anything is enqueued (pyz_fsvi_check is the same test on a bare shape, no device needed): a loss
 * other than PYZ_LOSS_MSE, a last layer of other than one unit or with softmax, k < 1, batch outside [1, batch_size],
 * n > 1024, D > 2048, t outside [1, 2^29), a null pointer.  PYZ_E_SHAPE: n > max_batch or k > max_particles of the plan.
 * A pivot of either factorisation that is not positive makes d_loss NaN, counts in the plan's sentinel (pyz_check_finite)
 * and leaves NaN in that particle's term; nothing is masked.  The workspace (the two float64 systems: k (n^2 + D^2) doubles)
 * is allocated on the first call, owned by the plan and counted by pyz_mlp_workspace_bytes. */
int pyz_fsvi_check(int n_layers, const int32_t *h_dims, const int32_t *h_acts, int loss, int k, int batch, int batch_size);
int pyz_fsvi_step(pyz_mlp *mlp, float *d_mu, float *d_particles, int k, float *d_adam_m, float *d_adam_v, const float *d_x,
                  const float *d_y, const int32_t *d_row_idx, int batch, int batch_size, const float *d_lo,
                  const float *d_hi, float lr, int64_t t, uint64_t seed, const float *d_xm, const float *d_noise,
                  const float *d_eps, double *d_alpha, float *d_stein, float *d_grad, float *d_xp, float *d_f,
                  float *d_loss, void *stream);

/* Batched symmetric positive-definite solve in float64 (the primitive of both FSVI terms; needs no plan): n_systems systems
 * d_a (n_systems, n, n) row-major (the lower triangle is read), d_rhs (n_systems, n).  One workgroup per system: in-place
 * lower Cholesky, forward and back substitution; d_rhs receives the solutions, d_a is scratch afterwards.  n <= 128 runs
 * inside LDS, larger systems in global memory.  d_fail (optional, int32[n_systems]): 1 where a pivot was not positive (that
 * solution is NaN-filled), else 0 -- a normal return.  1 <= n <= 2048, 1 <= n_systems <= 65535, else PYZ_E_INVALID. */
int pyz_spd_solve_f64(double *d_a, double *d_rhs, int n, int n_systems, int *d_fail, void *stream);

/* ---- R1: BayesianModel.predict (BayesianModel.py:106-129): S weight draws
 * d_weights (S, D) -> d_samples (S, n, out) with NaN -> 0, d_mean (n, out). */
int pyz_predict(pyz_mlp *mlp, const float *d_weights, int n_samples, const float *d_x, int n,
                float *d_samples, float *d_mean, void *stream);

/* The per-row moments of the same read-out, for callers that need the draws only through them
 * (Metrics.classification_uncertainty, visualisations/Metrics.py): d_mean (n, out) as pyz_predict writes it, bit for bit,
 * and d_m2 (n, out, out), d_m2[j][a][b] = sum_s p[s][j][a] * p[s][j][b] over the n_samples draws, p = pyz_predict's
 * samples (softmax applied where the last activation is softmax, NaN -> 0) -- which are never written: one kernel per
 * chunk of max_particles draws reads the last layer's outputs once and keeps the sums in registers.  Every element is a
 * sequential float32 sum in draw order (the same bits on every call and for every max_particles; d_m2 is symmetric bit
 * for bit).  Both outputs are required; rows >= n of neither are written; n <= max_batch.  out beyond ~13 000 (a row
 * no longer fits a compute unit's LDS) is refused with PYZ_E_SHAPE. */
int pyz_predict_moments(pyz_mlp *mlp, const float *d_weights, int n_samples, const float *d_x, int n,
                        float *d_mean, float *d_m2, void *stream);

/* ---- decision surfaces: what Plotter.plot_decision_boundaries / plot_uncertainty_area (visualisations/Plotter.py:54-78,
 * 100-135) need of a read-out on a dense 2-D grid, made and kept on the device.
 *
 * pyz_grid_rows writes rows [row0, row0 + n) of the n1 x n2 grid, mapped back to input space.  No plan is needed.  Row r
 * has i = r / n2, j = r % n2 (tf.meshgrid(indexing='ij') then reshape(-1), :132-133), u = a0 + (float)i * da,
 * v = b0 + (float)j * db, and d_out[r - row0][k] = u * B[k][0] + v * B[k][1] with B = d_basis, (d, 2) float32 row-major
 * (grid @ base_matrix^T, :134).  Every product and sum is rounded to float32 on its own (no contraction): a NumPy float32
 * restatement is equal bit for bit.  PYZ_E_INVALID, before the device is touched: a null pointer, n1 < 1, n2 < 1, d < 1,
 * n < 1, a row range outside the grid. */
int pyz_grid_rows(const float *d_basis, int d, float a0, float da, int n1, float b0, float db, int n2, int64_t row0,
                  int64_t n, float *d_out, void *stream);

/* The read-out of pyz_predict, keeping only (p = pyz_predict's sample value: softmax where the last activation is
 * softmax, NaN -> 0, never written):
 *   d_cols (n_samples, n), optional: d_cols[s][j] = p[s][j][column], bit for bit;
 *   d_mean (n, out), required (it carries the sums across chunks of draws): pyz_predict's mean, bit for bit;
 *   d_top float[n], d_cls int32[n], d_ent float[n], each optional, functions of the finished mean row q (out == 1: the
 *   pair (1 - m, m), the subtraction in float32, Plotter.py:37-39,49-51,68-70): top = max_a q_a, cls = the first index of
 *   the maximum (np.argmax), ent = -sum_a q_a * logf(q_a + 1e-5f), a sequential float32 sum in column order with every
 *   product and sum rounded on its own (:366), written raw: nan_to_num is the host's.
 * One kernel per chunk of max_particles draws, in place of pyz_predict's two; the bits do not depend on the chunking.
 * Rows >= n of no output are written.  n <= max_batch (PYZ_E_SHAPE); column in [0, out), n_samples >= 1, the required
 * pointers non-null (PYZ_E_INVALID); out beyond ~13 600 (a row no longer fits a compute unit's LDS): PYZ_E_SHAPE. */
int pyz_predict_surface(pyz_mlp *mlp, const float *d_weights, int n_samples, const float *d_x, int n, int column,
                        float *d_cols, float *d_mean, float *d_top, int32_t *d_cls, float *d_ent, void *stream);

/* ---- R2: the input gradient of Robustness.adversarial_robustness (visualisations/Robustness.py:115-144):
 * d_xgrad (n, dims[0]) = scale * sum_s d loss_s / d x over the n_samples draws d_weights (n_samples, D), loss_s =
 * draw s's mean loss over the n contiguous rows of d_x (no row gather; d_y as for pyz_mlp_loss_grad), summed inside
 * one GEMM over (draw, hidden unit) in a fixed order (the same bits on every call).  Optional: d_xadv (n, dims[0]) =
 * d_x + epsilon * sign(d_xgrad) with sign(0) = 0 and NaN kept (the FGSM step), d_loss (n_samples) = each draw's mean
 * loss.  Draws go through the plan in chunks of its max_particles; n <= max_batch.  A non-finite loss counts in the
 * plan's counter (pyz_check_finite); nothing is masked. */
int pyz_input_grad(pyz_mlp *mlp, const float *d_weights, int n_samples, const float *d_x, const void *d_y, int n,
                   float scale, float *d_xgrad, float epsilon, float *d_xadv, float *d_loss, void *stream);

/* ---- R3: the corrupted inputs of Robustness.mean_corruption_error / corruption_error / robustness_by_corruption /
 * corruption_robustness_by_severity (visualisations/Robustness.py:10-93 the corruption functions, :235-273 _error_rate,
 * _corrupt, _corrupt_regression), made on the device without PIL or skimage.  No plan is needed.
 * d_x (n, h, w, ch) float32, ch 1 or 3 -> d_out (n_sev, n, h * w * ch): block s holds severity severities[s] (a HOST
 * array, values 1..5, n_sev <= 5), one launch for all of them.  v = x / pixel_max; a one-channel image is replicated to
 * three channels (:260-266) and every kind works on three; c = the reference's table entry; clip is to [0, 1]:
 *   0 gaussian_noise  clip(v + c z)
 *   1 shot_noise      clip(K / c), K ~ Poisson(clip(v) c) by inversion from one uniform u:
 *                     p = exp(-lam); s = p; k = 0; while (u > s && k < 255) { ++k; p *= lam / k; s += p; }
 *   2 impulse_noise   skimage 's&p', salt_vs_pepper 0.5: flipped if u0 < c, then 1 if u1 < 0.5 else 0
 *   3 speckle_noise   clip(v + v c z)
 *   4 gaussian_blur   scipy.ndimage.gaussian_filter per channel, sigma = c, truncate 4, mode "nearest": radius
 *                     r = int(4 c + 0.5), weights exp(-0.5 k^2 / c^2) / their sum, indices clamped to the image, axis 0
 *                     then axis 1, taps summed from -r to r (r may exceed the image)
 *   5 contrast        clip((v - m) c + m), m the channel's mean over the image
 *   6 brightness      RGB -> HSV, V = clip(V + c), HSV -> RGB (skimage.color's formulas), clip
 *   7 saturate        RGB -> HSV, S = clip(S c0 + c1), HSV -> RGB, clip
 *   8 pixelate        PIL BOX down to (max(1, int(h c)), max(1, int(w c))), horizontal pass then vertical, NEAREST back up,
 *                     in float.  BOX along an axis of length in -> out: scale = in / out, center = (i + 0.5) scale,
 *                     lo = max(0, int(center - scale / 2 + 0.5)), hi = min(in, int(center + scale / 2 + 0.5)), source j in
 *                     [lo, hi) has weight 1 if -0.5 < (j - center + 0.5) / scale <= 0.5, normalised by the sum (float64
 *                     decisions).  NEAREST: source index min(small - 1, int((i + 0.5) small / in))
 *   9 gaussian_noise_regression  x + c z on every element of a row of any length: pass the length as w, h = ch = 1; no
 *                     replication, clip or quantisation, pixel_max is ignored
 * Kinds 0..8 with quantise = 1: each channel becomes the level floor(255 value) (np.uint8 at :270), a one-channel input
 * takes the mean of its three levels (:246), the result is multiplied by pixel_max / 255 -- with pixel_max = 255 the
 * reference's numbers.  quantise = 0: the value (or the channel mean of the values) times pixel_max, without the floor.
 * Noise: Philox stream PYZ_STREAM_CORRUPT (csrc/pyz_rng.h), step = 8 kind + severity, element ((i h + y) w + x) 3 + k of
 * the replicated tensor (kind 9: i w + j): a function of (seed, kind, severity, element) alone, so one severity called
 * alone gives the bits it has in a call with five.  PYZ_E_INVALID, with no device touched: ch outside {1, 3}, a severity
 * outside 1..5, n_sev outside 1..5, an unknown kind, an image whose two three-channel copies (2 * 3 * h * w floats, plus the
 * kernel's reduction row and pixelate's tap table) exceed the 160 KiB of LDS (64 x 64 fits). */
int pyz_corrupt_rows(const float *d_x, int64_t n, int h, int w, int ch, int kind, const int32_t *severities, int n_sev,
                     float pixel_max, int quantise, uint64_t seed, float *d_out, void *stream);

/* The scores of such read-outs (met.accuracy_score / met.root_mean_squared_error at Robustness.py:250-254), for `groups`
 * blocks of n rows at once: d_mean (groups, n, C) float32, the mean predictions.
 *   kind 0, classification: d_y int32[n] labels shared by every group; d_out int64[groups] = the rows whose predicted class
 *     differs from the label.  Predicted class: the first index of the maximum for C >= 2 (np.argmax), mean > 0.5 for C == 1.
 *   kind 1, regression: d_y float32 (n, C); d_out double[groups * C] = the sum over rows of (mean - y)^2, float64 sums per
 *     workgroup added in workgroup order (no floating-point atomics: the same bits on every call). */
int pyz_score_rows(const float *d_mean, int groups, int64_t n, int C, const void *d_y, int kind, void *d_out, void *stream);

/* ---- D1: one policy update of Deep-PILCO (Pyesian/dynamics/deep_pilco.py:247-326): a rollout of K particles through
 * the policy and K draws of a dynamics network, its cost, the cost's gradient with respect to the policy's parameters
 * and, when asked, one Keras-Adam update of them.  Both networks are Dense stacks in the flat parameter order:
 * policy dims (S, hidden..., A), dynamics dims (S + A, hidden..., S).  Hidden activations: linear / relu / tanh / sigmoid;
 * the policy's last layer may also be softmax; the dynamics' last layer must be linear.
 *   for t = 1..H, s = s_{t-1}:  a_i = policy(phi, s_i)  (the output itself: softmax probabilities, never an arg-max)
 *                               y_i = dynamics(W_i, [s_i, a_i])
 *                               m = mean_i y_i,  sd = sqrt(mean_i (y_i - m)^2),  s_t,i = m + sd * eps[t-1][i]
 *   cost = -mean_i r(s_0,i, 0) - sum over t in 1..H with t % freq == 0 of gamma^(t / freq) * mean_i r(s_t,i, t)
 * Rewards (dynamics/custom.py:6-18):
 *   PYZ_REWARD_CART  r = -s2 - s3 s2 + t (-s2^2 + 0.2095^2)              S >= 4
 *   PYZ_REWARD_ACB   r = 4 - 3 s0 - (s0 s2 - s1 s3) + s4^2              S >= 5
 * pyz_pilco_create refuses (PYZ_E_INVALID, no device touched) K < 2 (sd is identically 0 and the gradient NaN), a
 * dynamics net whose last layer is not linear or whose dims do not fit the policy's, and anything past the limits
 * K <= 256, S + A <= 64, layer widths <= 512, at most 8 layers per net, max_horizon <= 4096.  The handle owns the
 * tape of max_horizon steps (pyz_pilco_workspace_bytes).
 * pyz_pilco_policy_step: d_phi float32[D_pol]; d_W (K, D_dyn); d_s0 (K, S); d_eps (H, K, S) unit normals (the kernels draw
 * nothing: fill it with pyz_fill_normal, stream PYZ_STREAM_PILCO = 8 of csrc/pyz_rng.h); gamma the discount.  adam_t = 0: gradient only, d_phi
 * is not written and d_m / d_v may be NULL.  adam_t >= 1: m += (g - m)(1 - 0.9); v += (g^2 - v)(1 - 0.999);
 * phi -= lr sqrt(1 - 0.999^t) / (1 - 0.9^t) * m / (sqrt(v) + 1e-7).  Outputs: d_cost float32[1], d_grad float32[D_pol],
 * optional d_states (H + 1, K, S) and d_actions (H, K, A).  2 H + 3 launches; every sum runs in one fixed order, so the
 * bits are the same on every call.  use_graph != 0: the 2 H + 2 launches behind the first are captured once per (H, freq,
 * reward and every pointer argument) as one chain on `stream` and replayed.  PYZ_E_INVALID for a reward whose indices
 * exceed S or an unknown one, freq < 1, a null pointer; PYZ_E_SHAPE for H outside [1, max_horizon].  Nothing is launched
 * after a refusal.
 * pyz_pilco_create_layers is pyz_pilco_create with a kind and a gamma per policy layer (pyz_pilco_create: every layer
 * PYZ_PILCO_DENSE).  PYZ_PILCO_RBF is the RBF layer of deep_pilco.py:28-51, h[n] = exp(-gamma sum_k (x[k] - mean[k][n])^2):
 * its one variable `mean` (in, units) row-major takes in * units floats of phi at the layer's place, there is no bias, its
 * activation entry must be PYZ_ACT_LINEAR and gamma is a constant of the plan, not part of phi.  Refused (PYZ_E_INVALID, no
 * device touched): an unknown kind, an RBF as the last policy layer, a gamma that is not finite or not > 0, RBF units
 * outside [1, 512].  The dynamics net stays a Dense stack.
 * pyz_pilco_act: d_actions (N, A) = the policy of the plan on d_states (N, S) under d_phi, one launch, the arithmetic of
 * the rollout (its actions for a rollout's states are the rollout's actions bit for bit).  PYZ_E_INVALID for N < 1 or a
 * null pointer, before any launch. */
#define PYZ_REWARD_CART 0
#define PYZ_REWARD_ACB 1
#define PYZ_PILCO_DENSE 0
#define PYZ_PILCO_RBF 1
typedef struct pyz_pilco pyz_pilco;
int pyz_pilco_create(int n_policy_layers, const int32_t *h_policy_dims, const int32_t *h_policy_acts, int n_dynamics_layers,
                     const int32_t *h_dynamics_dims, const int32_t *h_dynamics_acts, int particles, int max_horizon,
                     pyz_pilco **out);
int pyz_pilco_create_layers(int n_policy_layers, const int32_t *h_policy_dims, const int32_t *h_policy_acts,
                            const int32_t *h_policy_kinds, const float *h_policy_gammas, int n_dynamics_layers,
                            const int32_t *h_dynamics_dims, const int32_t *h_dynamics_acts, int particles, int max_horizon,
                            pyz_pilco **out);
int pyz_pilco_destroy(pyz_pilco *plan);
int64_t pyz_pilco_workspace_bytes(const pyz_pilco *plan);
int pyz_pilco_policy_step(pyz_pilco *plan, float *d_phi, float *d_m, float *d_v, int64_t adam_t, const float *d_W,
                          const float *d_s0, const float *d_eps, int H, int freq, float gamma, int reward, float lr,
                          float *d_cost, float *d_grad, float *d_states, float *d_actions, int use_graph, void *stream);
int pyz_pilco_act(pyz_pilco *plan, const float *d_phi, const float *d_states, int N, float *d_actions, void *stream);

/* ---- noise: d_out[i] = mean + std * z_i, z from Philox stream (seed, stream, step).
 * (tf.random.normal at SGLD.py:67, HMC.py:171; tfp samplers at BBB.py:234-237,
 * SVGD.py:154, distributions/tf/TensorflowProbabilityDistribution.py:55-58.) */
int pyz_fill_normal(float *d_out, int64_t n, uint64_t seed, uint32_t stream_id, uint32_t step,
                    float mean, float std, void *stream);

/* n_rows draws of a vector Normal(d_loc, d_scale) (float32[len]) into columns [col0, col0 + len) of the
 * row-major (n_rows, row_stride) matrix d_out: the weight draws of BayesianModel._sample_weights
 * (BayesianModel.py:63-77) for Normal posteriors, made where pyz_predict reads them.  Draw r uses the
 * Philox counter (seed, stream_id, first_draw + r). */
int pyz_sample_normal_rows(float *d_out, int64_t n_rows, int64_t row_stride, int64_t col0, int64_t len,
                           const float *d_loc, const float *d_scale, uint64_t seed,
                           uint32_t stream_id, uint32_t first_draw, void *stream);

/* n_rows draws of SWAG's posterior (distributions/MultivariateNormalDiagPlusLowRank.py:32-41) into columns
 * [col0, col0 + len) of the row-major (n_rows, row_stride) matrix d_out:
 *   d_out[r][col0 + e] = d_mean[e] + d_diag[e] * z1(r, e) + factor * sum_{c < k} d_dev[c][e] * z2(r, c)
 * d_mean, d_diag float32[len] (d_diag is the scale of z1, as the reference writes it); d_dev (k, len) row-major, row c =
 * column c of the reference's deviation matrix; factor = sqrt(1 / (2 (k - 1))) is the caller's.  Draw r uses the Philox
 * counter (seed, stream_id, first_draw + r): z1(r, e) is its element e, z2(r, c) its element 4 * ceil(len / 4) + c.  The
 * sum over c is an ascending fmaf chain from 0, then fmaf(factor, sum, fmaf(diag, z1, mean)): the bits of an element do
 * not depend on n_rows, col0 or how a matrix is cut into calls.  1 <= k <= PYZ_LOWRANK_MAX_K, else PYZ_E_INVALID. */
#define PYZ_LOWRANK_MAX_K 256
int pyz_sample_lowrank_rows(float *d_out, int64_t n_rows, int64_t row_stride, int64_t col0, int64_t len,
                            const float *d_mean, const float *d_diag, const float *d_dev, int k, float factor,
                            uint64_t seed, uint32_t stream_id, uint32_t first_draw, void *stream);

/* d_out[r][col0 + e] = d_bank[d_idx[r]][e]: n_rows rows of the row-major (n_bank, len) matrix d_bank, picked by the
 * DEVICE indices d_idx (int32[n_rows]), into columns [col0, col0 + len) of the row-major (n_rows, row_stride) matrix
 * d_out -- the draws of distributions/Sampled.py:29-32 from samples that stay on the device.  The caller checks the
 * indices it uploads; a row whose index is outside [0, n_bank) is not written (and nothing is read for it). */
int pyz_gather_rows(float *d_out, int64_t n_rows, int64_t row_stride, int64_t col0, int64_t len,
                    const float *d_bank, int64_t n_bank, const int32_t *d_idx, void *stream);

/* ---- device memory for callers that have no allocator of their own (a TensorFlow / NumPy host process binding
 * this library from the reference's step(), INTEGRATION.md route B; torch-ROCm callers pass their tensors'
 * storage instead).  pyz_upload / pyz_download copy between a HOST buffer and device memory and return when
 * the host buffer may be reused / holds the data; pyz_sync waits for `stream`. */
int pyz_malloc(size_t bytes, void **d_out);
int pyz_free(void *d_ptr);
int pyz_upload(void *d_dst, const void *h_src, size_t bytes, void *stream);
int pyz_download(void *h_dst, const void *d_src, size_t bytes, void *stream);
int pyz_sync(void *stream);

/* ---- exchange step of the sharded SVGD run without a collective library ("verify a direct algorithm, else a
 * peer-write fallback"): every rank WRITES its rows straight into every peer's gathered matrix (peer-mapped memory over
 * xGMI, the caller's copies) and then its slot of the peer's flag array; a consumer parks this on the stream that reads the
 * gathered matrix: the stream goes on once d_flags[0 .. n) are all >= value (system-scope loads, one wave), i.e. once
 * every rank's rows of that step have landed.  Gives up after spin_limit polls without progress: *d_fail (optional) is set to
 * 1 and the stream goes on.  PYZ_E_INVALID for n outside [1, 64]. */
int pyz_wait_flags(const uint64_t *d_flags, int n, uint64_t value, int spin_limit, int *d_fail, void *stream);

/* ---- measurement hook (bench.py roofline leg): launch `iters` times ONE kernel of the
 * gradient step on the workspace left by the last pyz_mlp_loss_grad call with the same
 * arguments.  kind: 0 = k_dense_fwd of `layer` (G1), 1 = k_dense_bwd_data of `layer`,
 * 2 = k_wgrad_all, the weight gradients of ALL layers (G3; `layer` ignored), written to
 * d_grad (P, D). */
int pyz_bench_dense_kernel(pyz_mlp *mlp, int kind, int layer, const float *d_theta, int n_particles,
                           const float *d_x, const int32_t *d_row_idx, int batch, float *d_grad,
                           int iters, void *stream);

/* ---- diagnostic build only (-DPYZ_STAMPS, csrc/libpyz_stamps.so): copy the in-kernel
 * phase stamps {shader clock, 100 MHz clock} x 8 slots x 256 workgroups x 4 kernels to
 * h_out (uint64).  The shipped library returns PYZ_E_INVALID. */
int pyz_debug_stamps(uint64_t *h_out, int64_t n_words);

/* ---- diagnostic: the lane layout of v_mfma_f64_16x16x4_f64's result as probed on this device:
 * h_out512[4 l + r] = row, h_out512[256 + 4 l + r] = column of register r of lane l (k_svgd_gram_tile runs only
 * when it is row = l / 16 + 4 r, column = l % 16). */
int pyz_debug_mfma_f64_layout(int32_t *h_out512);

/* ---- conv nets: a convolutional front end ("stem") in front of a Dense stack -------------------------------------------
 * Keras Sequential [InputLayer] (Conv2D [MaxPooling2D])+ Flatten Dense+ as the reference's builder emits it
 * (utils.py:129-150) and its image script trains it (tests/tf_dataset_test.py:42-57).  Images and feature maps are NHWC
 * (channels_last), so Flatten is the identity on the buffer.  The flat vector holds, per Conv2D, the kernel
 * (kh, kw, cin, cout) row-major then the bias (cout) -- Keras's variable order --, then the Dense layers as above:
 * D_total = pyz_stem_param_count + pyz_mlp_param_count of the Dense plan, whose dims[0] is pyz_stem_feature_count and whose
 * max_batch / max_particles are the stem's.
 *
 * h_ops holds 6 int32 per op: {PYZ_STEM_CONV, filters, kh, kw, padding (0 valid, 1 same), activation (linear .. sigmoid)}
 * or {PYZ_STEM_POOL, ph, pw, 0, 0, 0}.  Strides and dilation are 1; `same` pads k - 1 in all, (k - 1) / 2 on top / left
 * (TensorFlow's rule); a pool has stride = size, padding valid (floor(H / ph) rows, the remainder dropped) and follows a
 * Conv2D; its winner is the first maximum in row-then-column order of the window, a NaN propagates.
 * PYZ_E_INVALID for an unknown op or field, PYZ_E_SHAPE for a kernel larger than the padded image, a pool larger than its
 * input, more than 4094 taps per filter or more than 2^24 output positions per launch -- all before a device is needed. */
#define PYZ_STEM_CONV 0
#define PYZ_STEM_POOL 1
typedef struct pyz_stem pyz_stem;
int pyz_stem_create(int in_h, int in_w, int in_c, int n_ops, const int32_t *h_ops, int max_batch, int max_particles,
                    pyz_stem **out);
int pyz_stem_destroy(pyz_stem *stem);
int64_t pyz_stem_param_count(const pyz_stem *stem);
int64_t pyz_stem_feature_count(const pyz_stem *stem);
int64_t pyz_stem_workspace_bytes(const pyz_stem *stem);

/* the stem alone: d_features (P, batch, F) from rows of d_x (images, H * W * C), particle p reading the stem's block at
 * d_theta + p * theta_stride; and, after a forward of the same batch, the stem's block of the gradient (written at
 * d_grad + p * grad_stride) from d_feature_grad (P, batch, F) = d loss / d features. */
int pyz_stem_forward(pyz_stem *stem, const float *d_theta, int64_t theta_stride, int n_particles, const float *d_x,
                     const int32_t *d_row_idx, int batch, float *d_features, void *stream);
int pyz_stem_backward(pyz_stem *stem, const float *d_theta, int64_t theta_stride, int n_particles, const float *d_x,
                      const int32_t *d_row_idx, int batch, const float *d_feature_grad, float *d_grad, int64_t grad_stride,
                      void *stream);

/* the whole net, d_theta (P, D_total): pyz_mlp_forward / pyz_mlp_loss_grad / pyz_sgd_step / pyz_swag_step / pyz_predict of
 * a conv net (same arguments, same results).  The gradient of the whole vector is formed in one (D_total) buffer and the
 * steps (one particle) run the unfused update kernels over it.  pyz_convnet_predict: d_m2 NULL = pyz_predict (d_samples
 * optional); d_m2 given = pyz_predict_moments (d_samples ignored).  A Dense plan with PYZ_LOSS_BCE is refused by every one
 * of them (PYZ_E_INVALID): BinaryCrossentropy is not built for conv nets. */
int pyz_convnet_forward(pyz_stem *stem, pyz_mlp *dense, const float *d_theta, int n_particles, const float *d_x,
                        const int32_t *d_row_idx, int batch, float *d_out, void *stream);
int pyz_convnet_loss_grad(pyz_stem *stem, pyz_mlp *dense, const float *d_theta, int n_particles, const float *d_x,
                          const void *d_y, const int32_t *d_row_idx, int batch, float *d_grad, float *d_loss, void *stream);
int pyz_convnet_sgd_step(pyz_stem *stem, pyz_mlp *dense, float *d_theta, const float *d_x, const void *d_y,
                         const int32_t *d_row_idx, int batch, float lr, float *d_loss, void *stream);
int pyz_convnet_swag_step(pyz_stem *stem, pyz_mlp *dense, float *d_theta, float *d_mean, float *d_sq_mean, float *d_dev_row,
                          const float *d_x, const void *d_y, const int32_t *d_row_idx, int batch, float lr, int64_t n,
                          int update_moments, float *d_loss, void *stream);
int pyz_convnet_predict(pyz_stem *stem, pyz_mlp *dense, const float *d_weights, int n_samples, const float *d_x, int n,
                        float *d_samples, float *d_mean, float *d_m2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PYZ_H */
