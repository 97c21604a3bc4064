/*
 * libffd -- C ABI of the MI355X-native frequency-domain diffusion sampler.
 *
 * This is the drop-in boundary for the sampling hot path of
 * NoakLiu/FastFourierDiffusion (`fdiff`).  The reference has no FFI layer of its
 * own (it is pure Python on stock PyTorch ops), so each entry point below names
 * the reference Python interface it replaces (file:line relative to the
 * reference repository root).  Signatures use only plain C types: pointers are
 * raw device (HBM) or host addresses, sizes are explicit, streams are passed as
 * `void*` (a `hipStream_t`; NULL = the default stream).  No torch types.
 *
 * Conventions
 *   - every function returns 0 on success and a negative ffd_status on failure;
 *     it never throws and never calls exit(); `ffd_last_error(ctx)` returns a
 *     human-readable message for the most recent failure on that context;
 *   - all device work is stream-ordered on the caller's stream: the functions
 *     enqueue kernels and return without synchronising (exceptions are noted);
 *   - I/O buffers are caller-owned and only borrowed for the stream-ordered
 *     call; weights are copied (and re-packed) into context-owned HBM;
 *   - one context per device; a context is not thread-safe, distinct contexts
 *     are independent: the only process-wide state is a per-device cache of FFT
 *     twiddle tables (the experiment knobs of ffd_tune -- kernel choice / tiling,
 *     never results -- are per calling thread);
 *   - tensors are dense row-major fp32: series X/score (B, L, C) with C
 *     innermost and L the Fourier / attention axis (score_models.py:87-90,
 *     fourier.py:12,24).
 */
#ifndef FFD_H
#define FFD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffd_ctx ffd_ctx;

typedef enum {
  FFD_OK = 0,
  FFD_ERR_INVALID = -1,     /* bad argument / shape (the reference's `assert`s, score_models.py:87-93) */
  FFD_ERR_UNSUPPORTED = -2, /* configuration this build has no kernel for (reference: NotImplementedError) */
  FFD_ERR_STATE = -3,       /* call order (e.g. forward before weights are finalised) */
  FFD_ERR_HIP = -4,         /* a HIP runtime call failed; message carries hipGetErrorString */
  FFD_ERR_NOMEM = -5
} ffd_status;

enum { FFD_MODEL_TRANSFORMER = 0, FFD_MODEL_LSTM = 1, FFD_MODEL_MLP = 2 };
/* No network: the exact score of a diffused Gaussian mixture (see ffd_mixture_score), an extension beyond the reference.
 * Weights: mixture.means (K L C), mixture.log_weights (K), mixture.variance (L C).  Every entry point that takes a score
 * model takes it; the E2-CRF cache is FFD_ERR_UNSUPPORTED, as for the other non-transformer kinds. */
enum { FFD_MODEL_MIXTURE = 3 };
enum { FFD_SDE_VP = 0, FFD_SDE_VE = 1 };

/* Model + scheduler hyper-parameters.
 * Replaces the constructor arguments of ScoreModule / LSTMScoreModule / MLPScoreModule
 * (src/fdiff/models/score_models.py:25-37, 444-455, 364-376) and of VPScheduler /
 * VEScheduler (src/fdiff/schedulers/sde.py:91-97, 169-175). */
typedef struct {
  int32_t kind;            /* FFD_MODEL_* */
  int32_t n_channels;      /* C */
  int32_t max_len;         /* L */
  int32_t d_model;         /* d   (8, 16, 24, 32, 48, 60, 64 or 72 in this build; d / n_head in {2,3,4,5,6,8}; any d for mlp) */
  int32_t n_head;          /* H   (ignored for lstm) */
  int32_t num_layers;      /* NL */
  int32_t dim_feedforward; /* F   (PyTorch default 2048, score_models.py:61-63); multiple of 64.  mlp: d_mlp (any >= 1).
                            * mixture: K, the number of components (>= 1); d_model, n_head, num_layers are ignored */
  int32_t sde;             /* FFD_SDE_* */
  double sde_a;            /* VP: beta_min   | VE: sigma_min */
  double sde_b;            /* VP: beta_max   | VE: sigma_max */
  int32_t fourier_noise_scaling; /* SDE.noise_scaling (sde.py:16,49) */
  double eps;              /* SDE.eps (sde.py:16) */
} ffd_model_desc;

/* E2-CRF cache configuration: the E2CRFCache kwargs the gate actually reads
 * (src/fdiff/utils/caching.py:28-47,131-181: K and R; tau_0, tau_warn, ... are
 * stored but never read by the reference). */
typedef struct {
  int32_t K;
  int32_t R;
} ffd_cache_cfg;

/* E2CRFCache.stats / get_cache_stats counters (caching.py:107-111, 599-653). */
typedef struct {
  int64_t recompute_count;
  int64_t cache_hit_count;
  int64_t current_step;
  int32_t table_allocated; /* k_cache_tensor is not None */
  int32_t reserved;
} ffd_cache_stats;

/* ---- lifetime ---------------------------------------------------------- */

/* Build a context on HIP device `device`.  Replaces module construction +
 * `.cuda()` (cmd/sample.py:68-77).  Fails with FFD_ERR_HIP if no gfx950 device
 * is usable: there is no CPU fallback. */
int ffd_create(ffd_ctx** out, const ffd_model_desc* desc, int device);
void ffd_destroy(ffd_ctx* ctx);
const char* ffd_last_error(const ffd_ctx* ctx);
/* Static description of the build ("libffd <ver> gfx950 ..."), usable without a device. */
const char* ffd_version(void);

/* ---- weights ----------------------------------------------------------- */

/* Copy one parameter (host or device pointer, `n` floats) into the context.
 * `name` is the reference state_dict key:
 *   pos_encoder.embedding.weight (L,d)   time_encoder.W ((d+1)/2)
 *   time_encoder.dense.{weight (d,d),bias}  embedder.{weight (d,C),bias}
 *   unembedder.{weight (C,d),bias}
 *   backbone.layers.{i}.self_attn.{in_proj_weight (3d,d),in_proj_bias,out_proj.weight,out_proj.bias}
 *   backbone.layers.{i}.{linear1,linear2}.{weight,bias}  backbone.layers.{i}.{norm1,norm2}.{weight,bias}
 *   backbone.{i}.{weight_ih_l0 (4d,d),weight_hh_l0 (4d,d),bias_ih_l0,bias_hh_l0}   (lstm)
 *   mixture.means (K L C)   mixture.log_weights (K)   mixture.variance (L C)         (mixture: these three and no others)
 * Replaces nn.Module.load_state_dict / load_from_checkpoint (cmd/sample.py:68-75). Synchronous. */
int ffd_load_weight(ffd_ctx* ctx, const char* name, const float* data, size_t n);
/* Validate that every parameter was supplied, apply the nn.Embedding(max_norm)
 * renormalisation to its fixed point (transformer.py:13-15) and
 * re-pack GEMM weights into MFMA fragment order.  Synchronous.
 * Mixture: FFD_ERR_INVALID for a missing tensor and for values ffd_host_mixture_check refuses. */
int ffd_finalize_weights(ffd_ctx* ctx);

/* ---- scheduler tables (host only; no device needed) --------------------- */

/* SDE.set_noise_scaling (sde.py:42-60): writes G[0..L). */
int ffd_host_noise_scaling(int max_len, int fourier_noise_scaling, float* G_out);
/* SDE.set_timesteps (sde.py:62-64): fp32 linspace(1, eps, n) and step_size = t[0]-t[1]. */
int ffd_host_timesteps(int n, double eps, float* ts_out, float* step_size_out);
/* E2CRFCache.determine_recompute_set (caching.py:131-181): the recompute set is
 * always the prefix [0, n); returns n (>=0) for `step`. */
int ffd_host_gate(int step, int max_len, int K, int R);
/* Static bound of one encoder layer's attention scores, from its weights alone (float64).  The layer's input is the
 * output of a LayerNorm with parameters ln_weight / ln_bias (d_model each), so every input row x has
 * |x| <= R = (sqrt(d_model) max|ln_weight| + |ln_bias|) (1 + 1e-4), and for head h
 *   bound_out[h] = (q_scale (sigma(W_q^h) R + |b_q^h|)) (sigma(W_k^h) R + |b_k^h|)  >=  q_scale |q . k|
 * for every query / key row of that head (W^h: the head's head_dim rows of in_proj_weight (3 d_model, d_model); sigma: an
 * upper bound of the spectral norm; q_scale: the factor folded into q, log2(e) / sqrt(head_dim) in the fused kernels).
 * Writes d_model / head_dim values.  ffd_finalize_weights evaluates it for every layer behind a norm2 (layers >= 1):
 * where no head exceeds the kernels' threshold, the fused attention kernels skip their per-launch measurement of the
 * same bound. */
int ffd_host_attn_score_bound(const float* in_proj_weight, const float* in_proj_bias, const float* ln_weight,
                              const float* ln_bias, int d_model, int head_dim, double q_scale, double* bound_out);

/* CU masks of `parts` stream partitions (hipExtStreamCreateWithCUMask) for a chip of n_cus compute units in n_xcds XCDs.
 * Mask bit b names CU b / n_xcds of XCD b % n_xcds (measured on MI355X, tools/partition_probe.py: 256 bits, 8 XCDs).
 *   FFD_CU_LAYOUT_SPREAD  part p owns CUs [p, p + 1) n_cus / (n_xcds parts) of EVERY XCD (the layout the sampling loops use);
 *   FFD_CU_LAYOUT_XCD     part p owns the whole XCDs [p, p + 1) n_xcds / parts.  The masks are well formed, but the driver
 *                         runs an XCD's share of a grid on ANY of its CUs when the mask names none of them, so streams made
 *                         from these masks overlap on the whole chip: kept for the record, not used.
 * masks_out: parts x ceil(n_cus / 32) words, part-major; the parts' masks are disjoint, cover bits [0, n_cus) and (SPREAD)
 * hold the same number of CUs of every XCD.  FFD_ERR_INVALID: a null pointer, a count < 1, n_cus not a multiple of n_xcds,
 * CUs per XCD (SPREAD) or XCDs (XCD) not a multiple of parts, an unknown layout. */
enum { FFD_CU_LAYOUT_SPREAD = 0, FFD_CU_LAYOUT_XCD = 1 };
int ffd_host_cu_masks(int n_cus, int n_xcds, int layout, int parts, uint32_t* masks_out);

/* ---- single operators (device pointers, stream ordered) ---------------- */

/* ScoreModule.forward / LSTMScoreModule.forward (score_models.py:79-119, 486-511)
 * without cache: score_out (B,L,C) <- model(x (B,L,C), t). All samples share `t`
 * (sampler.py:59-60). */
int ffd_score_forward(ffd_ctx* ctx, const float* x, float t, float* score_out, int B, void* stream);

/* ScoreModule.forward(batch, recompute_tokens, step, return_crf=True)
 * (score_models.py:79-194 + CachedTransformerEncoderLayer.forward,
 * cached_transformer.py:106-329).  `n_recompute` is |recompute_tokens| (always
 * the prefix [0,n), see ffd_host_gate).  Maintains the context's KV table
 * (caching.py:302-396) and counters.  crf_out (NL,L,d) may be NULL. */
int ffd_score_forward_cached(ffd_ctx* ctx, const float* x, float t, float* score_out, float* crf_out,
                             int B, int n_recompute, void* stream);

/* The same two forwards with PER-SAMPLE diffusion times: the reference evaluates
 * time_encoder(X, timesteps) per sample (score_models.py:102, transformer.py:77-91) and its own
 * unit test calls forward with mixed timesteps (tests/test_score_models.py:70).  `timesteps` is
 * a (B) fp32 device array; no host synchronisation.  n_recompute < 0: no cache (ffd_score_forward);
 * otherwise the cached forward for |recompute_tokens| = n_recompute (crf_out may be NULL). */
int ffd_score_forward_ts(ffd_ctx* ctx, const float* x, const float* timesteps, float* score_out, float* crf_out,
                         int B, int n_recompute, void* stream);

/* Scheduler hyper-parameters for the context-free scheduler operators below
 * (VPScheduler / VEScheduler constructor arguments, sde.py:91-97, 169-175). */
typedef struct {
  int32_t sde;      /* FFD_SDE_* */
  int32_t reserved;
  double a;         /* VP: beta_min  | VE: sigma_min */
  double b;         /* VP: beta_max  | VE: sigma_max */
} ffd_sde_desc;

/* VPScheduler.step / VEScheduler.step (sde.py:129-165, 215-246), in place on x (B,L,C).
 * Context-free, like the reference scheduler objects: G (L floats, device) is the
 * scheduler's noise scaling (ffd_host_noise_scaling uploaded by the caller).
 * `t` is timesteps[i] widened to double (sampler.py:96-98).  z (B,L,C) supplies the
 * N(0,1) draw; if NULL it is generated on device by Philox4x32-10 keyed by
 * (seed, step) and counted by the global element index (sample_offset*L*C + i), so
 * results do not depend on how a batch is sharded across GPUs. */
int ffd_sde_step(const ffd_sde_desc* sde, float* x, const float* score, const float* G, double t,
                 float step_size, const float* z, uint64_t seed, uint64_t sample_offset, int step, int B,
                 int L, int C, void* stream);

/* ---- probability-flow ODE steps (an extension: the reference integrates with Euler-Maruyama only) ----
 * Every VP / VE score model has a deterministic ODE with the SDE's marginals (Song et al. 2021).  With the forward SDE
 * dx = f(x,t) dt + g(t) diag(G) dw (f = -1/2 beta(t) x for VP, 0 for VE; beta(t), the VE sqrt_derivative and G exactly
 * as in ffd_sde_step) its drift is
 *     d(x,t) = f(x,t) - 1/2 (g(t) G_l)^2 s(x,t)
 * and one interval of width step_size towards smaller t is
 *     Euler:  x <- x - d(x,t) step_size
 *     Heun :  d1 = d(x,t);  xp = x - d1 step_size;  d2 = d(xp,t_next);  x <- x - (1/2 (d1 + d2)) step_size.
 * No noise is drawn.  Per element, each a separate fp32 rounding (no FMA contraction), like ffd_sde_step:
 *     g = cs G_l, g2 = g g, gs = g2 s, hgs = 0.5 gs, d = a x - hgs (VP) | -hgs (VE).
 * Context-free and stream ordered; all buffers (B,L,C) on the device, none of them may alias another.
 * FFD_ERR_INVALID before any device work: a null pointer, B, L, C < 1, step_size <= 0, aliased outputs. */
/* Euler, in place on x. */
int ffd_ode_step(const ffd_sde_desc* sde, float* x, const float* score, const float* G, double t, float step_size,
                 int B, int L, int C, void* stream);
/* Heun's predictor at the interval's start t: drift_out <- d1, x_pred_out <- xp.  x is not modified. */
int ffd_ode_heun_predict(const ffd_sde_desc* sde, const float* x, const float* score, const float* G, double t,
                         float step_size, float* x_pred_out, float* drift_out, int B, int L, int C, void* stream);
/* Heun's corrector at the interval's end t_next: score_pred = the score at (x_pred, t_next), drift = the predictor's
 * d1; x (the state the predictor read) is updated in place. */
int ffd_ode_heun_correct(const ffd_sde_desc* sde, float* x, const float* x_pred, const float* score_pred,
                         const float* drift, const float* G, double t_next, float step_size, int B, int L, int C,
                         void* stream);

/* ---- linear multistep ODE steps: second order at one score evaluation per interval (an extension) ----
 * Adams-Bashforth 2 on the drift above (FFD_SOLVER_ODE_AB2) and DPM-Solver++ 2M, the exponential two-step form on the
 * data prediction (FFD_SOLVER_DPMPP_2M; Lu et al. 2022), are ONE device operation.  With the interval's history quantity
 *     q = qa x + qb G_l^2 s
 * the update is, in increment form (coefficient rounding only touches the increment),
 *     x <- x + (cxm1 x + cn q + cp q_prev),    hist <- q
 * and the solvers differ in the five coefficients (qa, qb, cxm1, cn, cp), which the host computes in float64:
 *   FFD_SOLVER_ODE_AB2   (uniform grid of width step_size = h)  q = d(x,t): qa = a(t) (VP: -beta(t)/2, VE: 0),
 *                        qb = -cs(t)^2 / 2, cxm1 = 0; cn = -1.5 h, cp = 0.5 h with history, cn = -h, cp = 0 without.
 *   FFD_SOLVER_DPMPP_2M  (reads t_prev, t, t_next; step_size unused)  alpha(t), sigma(t) of the forward marginal (without
 *                        G), lambda = log(alpha / sigma), h = lambda(t_next) - lambda(t), r = (lambda(t) -
 *                        lambda(t_prev)) / h, c = -alpha(t_next) expm1(-h):  q = (x + sigma^2 G_l^2 s) / alpha, qa = 1 /
 *                        alpha, qb = sigma^2 / alpha, cxm1 = sigma(t_next) / sigma(t) - 1; cn = c (1 + 1 / (2 r)),
 *                        cp = -c / (2 r) with history, cn = c, cp = 0 without.  No lower-order final step.
 * The first interval of a trajectory has no history (have_prev == 0): cp = 0 and hist is written, never read.
 * ffd_host_multistep_coef: host only (no device needed), float64, coef_out[5] in the order above.  FFD_ERR_INVALID: a null
 * pointer, an unknown solver or SDE, times that are not strictly decreasing (t_prev is ignored when have_prev == 0),
 * step_size <= 0 for AB2, (DPM++) a time at which sigma is 0, a non-finite result. */
int ffd_host_multistep_coef(const ffd_sde_desc* sde, int solver, double t_prev, double t, double t_next, double step_size,
                            int have_prev, double* coef_out);
/* The step: coef (host, 5 doubles) is rounded once to fp32; per element, each a separate fp32 rounding (no FMA
 * contraction):  g2 = G_l G_l, u = g2 s, q = (qa x) + (qb u), inc = (cxm1 x) + (cn q), [have_prev: inc = inc + (cp
 * hist)], x = x + inc, hist = q.  Context-free and stream ordered; x and hist (B,L,C) are updated in place.
 * FFD_ERR_INVALID before any device work: a null pointer, B, L, C < 1, hist aliasing x or score, a non-finite
 * coefficient, coef[4] != 0 with have_prev == 0. */
int ffd_ode_multistep_step(float* x, const float* score, const float* G, float* hist, const double* coef, int have_prev,
                           int B, int L, int C, void* stream);

/* ---- Langevin corrector (an extension: predictor-corrector sampling, Song et al. 2021, Algorithms 4 / 5) ----
 * Forward SDE dx = f dt + g(t) diag(G) dw exactly as in ffd_sde_step.  One corrector step at time t on sample b, with
 * the score s = s(x, t) and a draw z ~ N(0, I):
 *     u = G_l^2 s                      (the score preconditioned by the SDE's noise covariance; G_l = 1: the paper's)
 *     w = G_l z                        (noise of the SDE's own covariance)
 *     n_u[b] = ||u[b]||_2,  n_w[b] = ||w[b]||_2                    (over the L C elements of sample b)
 *     FFD_LANGEVIN_NORM_SAMPLE:  eps[b] = 2 alpha (snr n_w[b] / n_u[b])^2                  (the paper's form)
 *     FFD_LANGEVIN_NORM_BATCH :  eps[b] = 2 alpha (snr mean_b(n_w) / mean_b(n_u))^2        (score_sde / diffusers)
 *     x <- x + eps[b] u + sqrt(2 eps[b]) w
 *     alpha = 1 (VE);  alpha = max(1 - beta(t) step_size, 0) (VP: score_sde's 1 - beta_i, clamped for coarse grids)
 *     n_u[b] == 0 (batch: mean_b(n_u) == 0):  eps = 0 and the sample is left as it is (never inf / NaN).
 * With G = 1 this is the published algorithm; with Fourier G it is Langevin preconditioned by diag(G^2), which leaves
 * the same marginal invariant.  The batch norm makes a sample depend on its batch; the sample norm does not, but its
 * stationary variance carries an O(1 / (L C)) bias.
 * Operation order.  Per element, every product / sum a separate fp32 rounding (no FMA contraction):
 *     g2 = G_l G_l, u = g2 s, w = G_l z;  x' = (x + eps u) + se w,  se = (float) sqrt(2 (double) eps).
 * Norms: the terms are the fp32 squares u u and w w; a row's C terms are added in fp64 with c ascending; a sample's L
 * row sums are added in fp64 in an order fixed by l alone (partial k = rows k, k + 256, ... in order, then a pairwise
 * tree that folds the upper half of the 256 partials onto the lower, 128, 64, ... 1); the square root is taken in
 * fp64; mean_b adds the B norms in the same fixed order over b and divides by B; eps = (2 alpha) (r r), r = (snr n_w) /
 * n_u in fp64, rounded once to fp32.  No atomics: the result is bit-identical from run to run, and n_u[b], n_w[b] do
 * not depend on B or on b.
 * z == NULL draws on the device: element i of sample b takes slot g & 3 of Philox block g >> 2, g = (sample_offset + b)
 * L C + i, under stream tag `tag`; the update REGENERATES the draw the norms measured, so no z buffer exists.
 * ffd_sample_batch_pc uses tag 0x80000000 + step * n_corrector + j (tags below 2^31 are the predictor's step indices,
 * 0xFFFFFFFD .. 0xFFFFFFFF are taken by the loss and the prior).
 * In place on x, context-free, stream ordered, no host synchronisation.  work: caller-owned device scratch of
 * ffd_langevin_work_bytes(B, L) bytes, 16-byte aligned, free again when the call's work on the stream is done.
 * eps_out: NULL or (B) floats, receives eps.
 * FFD_ERR_INVALID before any device work: a null pointer (z and eps_out excepted), B, L, C < 1, snr <= 0, step_size <= 0,
 * an unknown norm, x == score, a misaligned work. */
enum { FFD_LANGEVIN_NORM_BATCH = 0, FFD_LANGEVIN_NORM_SAMPLE = 1 };
size_t ffd_langevin_work_bytes(int B, int L);
int ffd_langevin_step(const ffd_sde_desc* sde, float* x, const float* score, const float* G, double t, float step_size,
                      float snr, int norm, const float* z, uint64_t seed, uint64_t sample_offset, uint32_t tag, int B,
                      int L, int C, float* eps_out, void* work, void* stream);

/* ---- conditional sampling by replacement (an extension: Song et al. 2021, Appendix I.2; score_sde's
 * get_inpaint_update_fn) ----
 * One projection of the state x (B,L,C) onto an observation at time t, in place.  The observation is noised to the
 * forward SDE's marginal at t, as ffd_sm_perturb forms it,
 *     y_t = mc obs + (sigma G_l) z
 *     VP: lmc = -0.25 t^2 (b - a) - 0.5 t a, mc = exp(lmc), sigma = sqrt(-expm1(2 lmc));  VE: mc = 1, sigma = a (b/a)^t
 *     noiseless != 0: mc = 1, sigma = 0, y_t = obs, and no draw is read or generated
 * (the coefficients formed on the host in double and rounded once to fp32), and blended into x under a mask that lives
 * on the TIME axis (1 = observed, fractional values blend), in difference form:
 *     FFD_COND_FREQUENCY  x <- x + dft( mask (.) idft( (y_t - x) (.) std ) ) / std      (x, obs: packed ortho spectra)
 *     FFD_COND_TIME       x <- x + mask (.) (y_t - x)                                   (pointwise; std must be NULL)
 * The standardization mean cancels in the difference; an all-zero mask adds exact zeros (x is untouched); the unobserved
 * components take no round trip.  Unobserved time points of the series behind `obs` may hold anything finite: by
 * linearity the fill reaches the result only through rounding.
 *   obs, mask  (obs_batch, L, C), obs_batch = 1 (shared by the batch) or B;  mask values in [0, 1]
 *   std        NULL or (L, C), the dataset's feature_std, > 0 (the caller's contract, as for ffd_dft_standardize)
 *   z          NULL or (B, L, C) injected draws.  NULL draws on the device: element i of sample b takes slot g & 3 of
 *              Philox block g >> 2, g = (sample_offset + b) L C + i over the packed layout, under stream tag `tag`:
 *              the counting of ffd_sde_step and ffd_langevin_step, so a shard draws what the unsharded call draws.
 * Operation order.  Per packed element, every product / sum a separate fp32 rounding (no FMA contraction):
 *     sg = sigma G_l;  y = (mc obs) + (sg z)  (noiseless: y = obs);  d = y - x;  d = d std (std given)
 *   time domain:  x' = x + mask d.
 *   frequency domain:  the Hermitian image of d goes through the inverse butterflies; w = v_l / sqrt(L) per time point,
 *   then m = mask w; the forward butterflies; per packed element X = V / sqrt(L), X = X / std (std given), x' = x + X.
 *   The butterflies are those of ffd_idft / ffd_dft at this length (powers of two: the half-length real transform).
 * One launch: a workgroup owns a sample's (L x channel-group) slab in LDS for both transforms.  x, obs and z are read
 * once from HBM, the mask once at its point of use, x is re-read (L2) for the final sum and written once.
 * Context-free, stream ordered, no host synchronisation, no atomics: bit-identical from run to run, and a sample's
 * result does not depend on B or on its place in the batch.  obs, mask, std and z are not modified.
 * L: frequency domain see "Supported transform lengths" (2 <= L <= 4096); the time domain takes any L >= 1.
 * FFD_ERR_INVALID before any device work: a null pointer (z and std excepted), B, L, C < 1, obs_batch not 1 or B, an
 * unknown domain, std with the time domain, x aliasing obs, mask or z; then FFD_ERR_UNSUPPORTED for an unknown SDE or a
 * frequency-domain length outside its set.
 * ffd_sample_batch_cond uses tag 0xC0000000 + step * (n_corrector + 1) + k. */
enum { FFD_COND_FREQUENCY = 0, FFD_COND_TIME = 1 };
int ffd_cond_project(const ffd_sde_desc* sde, float* x, const float* obs, const float* mask, const float* std,
                     const float* G, double t, int noiseless, const float* z, uint64_t seed, uint64_t sample_offset,
                     uint32_t tag, int obs_batch, int domain, int B, int L, int C, void* stream);

/* ---- the forward transition of the SDE (an extension: the re-noising step of resampled conditional sampling, see
 * ffd_sample_batch_resample) ----
 * For 0 <= s <= t the forward SDE of ffd_sde_step takes x_s to
 *     x_t = a x_s + (sg G_l) z,      z ~ N(0, I)
 *     VP: a = exp(lmc(t) - lmc(s)), sg = sqrt(-expm1(2 (lmc(t) - lmc(s)))), lmc as in ffd_cond_project
 *     VE: a = 1, sg = sqrt(sigma(t)^2 - sigma(s)^2), sigma(t) = a_ve (b / a_ve)^t
 * the same SDE, G and coefficient conventions as ffd_cond_project, ffd_sm_perturb and ffd_sde_step; s = 0 gives the
 * marginal's (mc, sigma) for VP.  Transitions compose: a(r,t) = a(r,s) a(s,t), sg(r,t)^2 = a(s,t)^2 sg(r,s)^2 + sg(s,t)^2.
 * ffd_host_transition_coef: host only (no device needed), float64, coef_out = (a, sg); s == t gives exactly (1, 0).
 * FFD_ERR_INVALID: a null pointer, non-finite times, s < 0, t < s; then FFD_ERR_UNSUPPORTED for an unknown SDE. */
int ffd_host_transition_coef(const ffd_sde_desc* sde, double s, double t, double coef_out[2]);
/* The operator, in place on x (B,L,C).  The coefficients are formed on the host in double and rounded once to fp32; per
 * element, every product / sum a separate fp32 rounding (no FMA contraction):  x' = (a x) + ((sg G_l) z).
 * z == NULL draws on the device: element i of sample b takes slot g & 3 of Philox block g >> 2, g = (sample_offset + b)
 * L C + i, under stream tag `tag` -- the counting of ffd_sde_step, ffd_langevin_step and ffd_cond_project, so a shard
 * draws what the unsharded call draws.  With sg == 0 (fp32) no draw is read or generated and x' = a x; with a == 1 as
 * well nothing is launched and x is untouched bit for bit.  One float4 of x (and z) per thread and iteration where
 * C % 4 == 0, the buffers are 16-byte aligned and the element offset is a multiple of 4 (one Philox block per float4);
 * a scalar kernel with the same bits otherwise.  8 B of HBM traffic per element with device draws, 12 B with z.
 * Context-free, stream ordered, no host synchronisation, no atomics: bit-identical from run to run, and a sample's
 * result does not depend on B or on its place in the batch.  z and G are not modified.
 * FFD_ERR_INVALID before any device work: a null pointer (z excepted), B, L, C < 1, t < s, s < 0, non-finite times, x
 * aliasing z; then FFD_ERR_UNSUPPORTED for an unknown SDE.
 * ffd_sample_batch_resample uses tag 0xE0000000 + q for transition q. */
int ffd_forward_transition(const ffd_sde_desc* sde, float* x, const float* G, double s, double t, const float* z,
                           uint64_t seed, uint64_t sample_offset, uint32_t tag, int B, int L, int C, void* stream);

/* ---- the closed-form score of a diffused Gaussian mixture (an extension: the "optimal denoiser" every trained score
 * network approximates; the backbone behind FFD_MODEL_MIXTURE) ----
 * Data distribution p_0 = sum_i w_i N(mu_i, diag(v)): means (K, L, C), log_weights (K), one shared per-coordinate
 * variance (L, C) >= 0 (NULL: v = 0, the empirical distribution of the rows of `means`).  Under the forward marginal
 * x_t = alpha(t) x_0 + sigma(t) G_l z of the SDE (alpha, sigma as in ffd_cond_project; G as in ffd_sde_step), per row
 * of x (B, L, C):
 *     c_lc    = alpha^2 v_lc + sigma^2 G_l^2
 *     logit_i = log w_i - 1/2 sum_lc (x_lc - alpha mu_i,lc)^2 / c_lc
 *     r       = softmax_i(logit)
 *     d_lc    = alpha sum_i r_i mu_i,lc - x_lc,        score_out = d / c.
 * Row b reads its time from t[b * t_stride] (device fp32; t_stride 0: one time shared by the batch, 1: per sample --
 * one code path, the same bits).  The time is widened to double; alpha and sigma^2 are formed in double (VP: sigma^2 =
 * -expm1(2 log alpha)) and rounded once.  The logits are evaluated in DIFFERENCE form in fp32 -- t = x - alpha mu (one
 * FMA), then sum t (t / c) -- never as |x|^2 - 2 x . alpha mu + |alpha mu|^2, which cancels catastrophically at small t
 * (1.6e-4 of the data scale against 5e-7).  The softmax subtracts the running maximum: a component
 * with log w = -inf is ignored exactly, logits of -1e8 and below give no NaN or Inf (the nearest component wins), K = 1
 * works.  sum_i r_i mu_i runs on the fp32 matrix cores (exact fp32).
 * Launches: rows in tiles of 16 x components in slices of 512 (ffd_mixture_tiling), each leaving (max, sum, weighted sum)
 * per row in `work`; then one merge launch combines the slices in ascending order.  No atomics: bit-identical from run
 * to run; the tiling depends on K and L C alone, so a row's result does not depend on B or on its place in the batch.
 * work: device scratch of at least ffd_mixture_work_floats(B, K, L, C) floats (0 for a shape the call refuses), free
 * again when the call's work on the stream is done.  score_out may be x.  Context-free, stream ordered, no host
 * synchronisation.  c must be > 0 (t > 0, G != 0).
 * FFD_ERR_INVALID before any device work: a null pointer (variance excepted), B, K, L, C < 1, t_stride not 0 or 1,
 * work_floats too small; FFD_ERR_UNSUPPORTED: an unknown SDE, L * C > 1024, K > 33 million, B * L * C >= 2^31.
 * The values are the caller's contract here; ffd_host_mixture_check (host arrays; what ffd_finalize_weights applies)
 * returns FFD_ERR_INVALID for a non-finite mean, a negative or non-finite variance, a NaN or +inf log-weight, or
 * log-weights that are all -inf, and FFD_ERR_UNSUPPORTED for L * C over the limit. */
size_t ffd_mixture_work_floats(int B, int K, int L, int C);
int ffd_mixture_score(const ffd_sde_desc* sde, const float* x, const float* t, int t_stride, const float* means,
                      const float* log_weights, const float* variance, const float* G, float* score_out, int B, int K,
                      int L, int C, float* work, size_t work_floats, void* stream);
int ffd_host_mixture_check(const float* means, const float* log_weights, const float* variance, int K, int L, int C);
/* The vector-Jacobian product of that score with respect to x: out = J^T v, J = d score / d x, v and out (B, L, C).
 * J is symmetric, J_jk = alpha^2 Cov_r(mu_j, mu_k) / (c_j c_k) - delta_jk / c_j, so with q = v / c
 *     J^T v = (alpha^2 / c) (.) (sum_i r_i mu_i p_i - m sum_i r_i p_i) - q,   p_i = (mu_i - x / alpha) . q,   m = sum_i r_i mu_i
 * (the covariance does not see the shift inside p_i, and p_i = -(x - alpha mu_i) . q / alpha reuses the difference the
 * logit forms).  A pass of its own with the tiling, the online softmax and the slice order of ffd_mixture_score: it
 * carries sum e p and, on the fp32 matrix cores, sum e p mu next to that call's sums, so it is bit-identical from run
 * to run and a row's result does not depend on B.  work: at least ffd_mixture_vjp_work_floats(B, K, L, C) floats (0 for
 * a shape the call refuses).  out may be v or x.  Arguments, limits and error codes as ffd_mixture_score (v must not be
 * NULL). */
size_t ffd_mixture_vjp_work_floats(int B, int K, int L, int C);
int ffd_mixture_score_vjp(const ffd_sde_desc* sde, const float* x, const float* t, int t_stride, const float* means,
                          const float* log_weights, const float* variance, const float* G, const float* v, float* out,
                          int B, int K, int L, int C, float* work, size_t work_floats, void* stream);
/* Host only: the kernel's rows per tile, components per tile, components per slice and the largest L * C (any pointer
 * may be NULL). */
int ffd_mixture_tiling(int* row_tile, int* comp_tile, int* slice, int* max_dim);

/* ---- reconstruction guidance (an extension: Ho et al. 2022, Chung et al. 2023 "DPS", Kollovieh et al. 2023
 * "observation self-guidance"; the conditioning that needs the gradient through the score model) ----
 * At time t, with alpha(t), sigma(t) as in ffd_cond_project, c_l = sigma^2 G_l^2 and s = score(x, t):
 *     x0hat = (x + c (.) s) / alpha                                   Tweedie's denoised estimate
 *     r     = mask (.) (x0hat - obs)                                  FFD_COND_TIME
 *     r     = mask (.) idft((x0hat - obs) (.) std)                    FFD_COND_FREQUENCY (std may be NULL)
 *     loss  = 1/2 sum r^2                                             per sample
 *     u     = d loss / d x0hat = mask (.) r                           time domain
 *     u     = std (.) W (.) dft(mask (.) r)                           frequency domain
 *     g     = grad_x loss = (u + J^T (c (.) u)) / alpha,  J = d s / d x
 *     s~    = s - lambda g,   lambda(t) = scale / (obs_var + rho sigma^2 / (alpha^2 + sigma^2))
 * The packed layout is not orthonormal: a bin other than DC (and Nyquist, even L) appears once where the Hermitian
 * image holds it twice, so the adjoint of idft is W (.) dft with W = 1 on the DC row, 1 on the Nyquist row of an even L
 * and 2 on every other packed row (real and imaginary parts alike).
 *
 * ffd_guide_seed writes u and v = c (.) u, the cotangent of the score model's input VJP (ffd_mixture_score_vjp,
 * ffd_train_input_vjp).  One launch: a workgroup owns a sample's (L x channel-group) slab in LDS for both transforms --
 * the Hermitian image, the butterflies and the 1 / sqrt(L) factors of ffd_cond_project's general-length kernel, at
 * every length -- and walks the sample's channel groups in order.  Per packed element, every product / sum a separate
 * fp32 rounding: c = sigma^2 (G_l G_l); x0hat = (x + c s) / alpha; d = x0hat - obs; d = d std (std given); r = mask w
 * (w = d in the time domain, the scaled inverse transform otherwise); u = mask r, or (V / sqrt(L)) W std behind the
 * forward transform; v = c u.  alpha and sigma^2 are formed on the host in double at t and rounded once (VE: alpha = 1).
 *   loss_out   NULL or B doubles: 1/2 sum r^2 in fp64, per-thread partial sums in a fixed element order, then a fixed
 *              tree: bit-identical from run to run
 *   x0hat_out  NULL or (B, L, C): the denoised estimate in the domain of x
 * obs, mask, std, obs_batch, domain as in ffd_cond_project.  A zero mask gives exact zeros and loss 0.  Context-free,
 * stream ordered, no host synchronisation, no atomics; a sample's result does not depend on B, on its place in the batch
 * or on obs_batch.
 * FFD_ERR_INVALID before any device work: a null pointer (std, loss_out and x0hat_out excepted), B, L, C < 1, obs_batch
 * not 1 or B, an unknown domain, std with the time domain, a non-finite or negative t, an output aliasing an input or
 * another output; then FFD_ERR_UNSUPPORTED for an unknown SDE or a frequency-domain length outside ffd_cond_project's. */
int ffd_guide_seed(const ffd_sde_desc* sde, const float* x, const float* score, const float* obs, const float* mask,
                   const float* std, const float* G, double t, int obs_batch, int domain, int B, int L, int C,
                   float* u_out, float* v_out, double* loss_out, float* x0hat_out, void* stream);
/* score_out = score - coef ((u + jtv) / alpha), pointwise over n elements, every product / sum / quotient a separate
 * fp32 rounding; score_out may be score.  FFD_ERR_INVALID: a null pointer, n < 1, alpha not finite or 0, coef not
 * finite. */
int ffd_guide_combine(const float* score, const float* u, const float* jtv, float alpha, float coef, float* score_out,
                      size_t n, void* stream);
/* Host only, float64: coef_out = (alpha(t), sigma(t)^2, lambda(t)).  FFD_ERR_INVALID: a null pointer, a non-finite or
 * negative t, scale, obs_var or rho, or a zero denominator; then FFD_ERR_UNSUPPORTED for an unknown SDE. */
int ffd_host_guide_coef(const ffd_sde_desc* sde, double t, double scale, double obs_var, double rho, double coef_out[3]);

/* SDE.prior_sampling (sde.py:79-87, 125-127): x <- G (.) z  (VE: * sigma_max);
 * z == NULL draws on device (Philox stream tag 0xFFFFFFFF). */
int ffd_prior(const ffd_sde_desc* sde, float* x, const float* z, const float* G, uint64_t seed,
              uint64_t sample_offset, int B, int L, int C, void* stream);

/* ---- log-likelihoods through the probability-flow ODE (an extension: Song et al. 2021, section 4.3 / appendix D.2) ----
 * Forward SDE and drift as in ffd_sde_step / ffd_ode_step: d(x,t) = a(t) x - 1/2 (cs(t) G_l)^2 s(x,t), a = -beta(t)/2 (VP)
 * or 0 (VE).  Along the ODE's solution from eps up to T = 1, by the instantaneous change of variables,
 *     log p_eps(x(eps)) = log p_T(x(1)) + integral of v dt,      v(x,t) = a(t) L C - 1/2 cs(t)^2 tr(diag(G^2) ds/dx).
 * No gradient of the network exists: the trace is estimated by Hutchinson probes with a central finite difference of the
 * score.  With probes eps_1 .. eps_k of shape (B, L, C), w_m = G_l eps_m, h = fd_rel sigma(t) (sigma: the marginal's
 * standard deviation without G, as in ffd_cond_project),
 *     tr ~ (1/k) sum_m sum_lc w_m (s(x + h w_m, t) - s(x - h w_m, t)) / (2 h),
 * which uses tr(G^2 J) = E[(G eps)^T J (G eps)]: the perturbation has the SDE's own noise covariance.  eps_j = sqrt(D) e_j
 * with k = D = L C makes the sum the exact trace (of the finite difference).
 * One divergence evaluation is ffd_loglik_perturb, the caller's score evaluation at the stacked batch, ffd_loglik_tail.
 * Rounding contract.  Per element, each product / sum its own fp32 rounding (no FMA contraction):
 *     w = G_l eps, hw = h w, x+ = x + hw, x- = x - hw;        diff = s+ - s-, term = w diff.
 * A sample's terms are added in fp64 in an order fixed by the probe index m and the element index i = l C + c alone:
 * partial p (0 .. 255) adds, for m ascending, the terms of elements p, p + 256, ... in ascending order, then the 256
 * partials go through a pairwise tree that folds the upper half onto the lower (128, 64, ... 1).  No atomics: bit-
 * identical from run to run, independent of B and of the sample's place in the batch.  In fp64, with a(t), cs(t) the
 * DOUBLE values ffd_ode_step rounds to fp32 and h the fp32 step widened:
 *     tr = sum / ((2 h) k),    v = a(t) (L C) + (-1/2 cs(t)^2) tr.
 * The state moves with ffd_ode_step's per-element rounding and the sign of an UPWARD step of width dt (fp32: (float)dt):
 *     FFD_LOGLIK_EULER    x <- x + d dt;                                   delta[b] <- delta[b] + dt v
 *     FFD_LOGLIK_PREDICT  drift <- d1 = d(x,t), x_pred <- x + d1 dt;       v1[b] <- v              (x, delta untouched)
 *     FFD_LOGLIK_CORRECT  (score_stack: at x_pred and t = the interval's end)
 *                         x <- x + (1/2 (d1 + d(x_pred,t))) dt;            delta[b] <- delta[b] + (dt / 2) (v1[b] + v)
 * delta, v1, v_out: (B) doubles on the device; dt in double for delta.  The drift reads block 0 of the score stack.
 * Probes.  `probes` (n_probes, B, L, C): injected, any finite values.  NULL: Rademacher draws from the Philox plan of
 * ffd_sde_step -- the word of global element g = (sample_offset + b) L C + i is slot g & 3 of block g >> 2 under (seed,
 * tag0 + m) for probe m; eps = +1 if bit 31 of the word is clear, else -1.  The tail REGENERATES what the perturbation
 * drew, so no probe buffer exists.  ffd_loglik_batch uses tag0 = 0xF0000000 + e n_probes for divergence evaluation e
 * (Euler: e = j for interval j; Heun: e = 2 j at the interval's start, 2 j + 1 at its end); the largest e n_probes + m of a
 * run must stay below 0x0FFFFFF0, which keeps the family clear of the reserved 0xFFFFFFFD .. 0xFFFFFFFF.  The family
 * 0xF0000000 .. overlaps the transition family 0xE0000000 + q of ffd_sample_batch_resample from q = 2^28 on: the two
 * entries never draw in one run (a likelihood draws probes only, a resampled run no probes), so no draw is shared.
 * Stacked batch: block 0 = x, block 2 m - 1 = x + h w_m, block 2 m = x - h w_m for m = 1 .. n_probes, (1 + 2 n_probes) B
 * rows of (L, C).
 * ffd_prior_logp: logp_out[b] = sum_lc log N(x; 0, (sigma_p G_l)^2), sigma_p = 1 (VP) or sigma_max (VE): the density
 * ffd_prior draws from.  Per element sg = sigma_p G_l, q = x / sg, term = (-0.5 (q q)) - (float)(log sg + log(2 pi) / 2),
 * each its own fp32 rounding (the logarithm in fp64, rounded once); the sum in fp64 in the order above (one "probe").
 * ffd_host_loglik_h: host only; *h_out = (float)(fd_rel sigma(t)) with sigma in double.
 * All three device operators: context-free, stream ordered, no host synchronisation, one launch each (one workgroup per
 * sample in the tail and the prior).  FFD_ERR_INVALID before any device work: a null pointer (probes, v_out and the
 * buffers a stage does not use excepted), B, L, C < 1, n_probes < 1, h, fd_rel or dt that is <= 0 or non-finite, a
 * negative or non-finite t, an unknown stage or SDE, a written buffer that shares an address with another buffer of the
 * call; then FFD_ERR_UNSUPPORTED for (1 + 2 n_probes) B L C >= 2^31. */
enum { FFD_LOGLIK_EULER = 0, FFD_LOGLIK_PREDICT = 1, FFD_LOGLIK_CORRECT = 2 };
int ffd_host_loglik_h(const ffd_sde_desc* sde, double t, double fd_rel, float* h_out);
int ffd_prior_logp(const ffd_sde_desc* sde, const float* x, const float* G, double* logp_out, int B, int L, int C,
                   void* stream);
int ffd_loglik_perturb(const float* x, const float* G, float h, int n_probes, const float* probes, uint64_t seed,
                       uint64_t sample_offset, uint32_t tag0, float* stack_out, int B, int L, int C, void* stream);
int ffd_loglik_tail(const ffd_sde_desc* sde, int stage, float* x, float* x_pred, float* drift, const float* score_stack,
                    const float* G, double t, double dt, float h, int n_probes, const float* probes, uint64_t seed,
                    uint64_t sample_offset, uint32_t tag0, double* delta, double* v1, double* v_out, int B, int L, int C,
                    void* stream);

/* ---- Supported transform lengths ----
 * Every Fourier entry point keeps a sample's slab and the twiddle table in one workgroup's 160 KiB of LDS, which
 * sets the lengths it takes:
 *   ffd_dft, ffd_idft, ffd_dft_standardize, ffd_unstandardize_idft,
 *   ffd_localization (and _bench), ffd_spectral_profile:  L a power of two up to 8192, or any other L up to 6826
 *                                                         (6827 .. 8191 do not fit next to their twiddle table);
 *   ffd_fresca, ffd_freq_decompose,
 *   ffd_cond_project (FFD_COND_FREQUENCY; and so
 *   ffd_sample_batch_cond):                               the same set up to L = 4096, L >= 2;
 *   ffd_smooth_frequency:                                 odd L up to 2047 (its L x L kernel).
 * Any number of channels: they are split over workgroups down to one channel each.  A length outside its set is
 * FFD_ERR_UNSUPPORTED, returned before any device call (no allocation, no launch), after the FFD_ERR_INVALID
 * argument checks; the matching *_work_bytes is 0 for exactly the shapes the call refuses. */

/* fdiff.utils.fourier.dft / idft (fourier.py:8-52, 55-94): packed ortho rFFT and
 * its inverse along dim 1 of (B,L,C).  `in` and `out` may not alias. Context-free.
 * L: see "Supported transform lengths". */
int ffd_dft(const float* in, float* out, int B, int L, int C, void* stream);
int ffd_idft(const float* in, float* out, int B, int L, int C, void* stream);
/* The runner-side wrappers around them, fused into the same kernel (no extra pass over the data):
 *   ffd_unstandardize_idft  cmd/sample.py:107-113   out = idft(in * std + mean)   (sampled spectra -> time series)
 *   ffd_dft_standardize     src/fdiff/dataloaders/datamodules.py:42-43,61-62   out = (dft(in) - mean) / std
 * mean / std: (L, C) fp32 on the device (DiffusionDataset.feature_mean / feature_std), broadcast over B. */
int ffd_unstandardize_idft(const float* in, float* out, const float* mean, const float* std, int B, int L, int C,
                           void* stream);
int ffd_dft_standardize(const float* in, float* out, const float* mean, const float* std, int B, int L, int C,
                        void* stream);

/* PositionalEncoding.forward (transformer.py:17-29): out = x + weight[arange(L)] for x (B,L,D); like
 * nn.Embedding(max_norm) the looked-up rows of `weight` (L,D, device) are renormalised IN PLACE first
 * (rows with ||w|| > max_norm scaled by max_norm/(||w||+1e-7); max_norm <= 0 disables it). */
int ffd_positional_encoding(const float* x, float* weight, float* out, int B, int L, int D, float max_norm,
                            void* stream);
/* GaussianFourierProjection.forward (transformer.py:77-91), use_time_axis=True:
 * out[b,l,:] = x[b,l,:] + dense([sin(2 pi t_b W), cos(2 pi t_b W)][:D]); timesteps (B) fp32 on device,
 * temb_work = B*D floats of scratch.  L = 1 gives the use_time_axis=False form. */
int ffd_time_encoding(const float* x, const float* timesteps, const float* W, const float* dense_w,
                      const float* dense_b, float* temb_work, float* out, int B, int L, int D, void* stream);

/* FreSca spectral scaling (fdiff.utils.fresca.frequency_scale / apply_fresca_to_score,
 * fresca.py:111-268, 3-D case): out = irfft((low*[k<=Rc] + high*[k>Rc]) (.) rfft(in)) along dim 1.
 * strategy 0 "spatial": Rc = cutoff_ratio * (L/2+1); 1 "energy": Rc = first k whose cumulative
 * batch-mean |X_k| reaches cutoff_ratio * total (fresca.py:46-58; a batch-wide statistic, reduced
 * on the device in a fixed order -- no host sync).  `work` = B*C*(L/2+1) + 4 floats of scratch.
 * Context-free; in != out.  low == high == 1 is the caller's early exit (fresca.py:137-138).
 * 2 <= L <= 4096 within the supported transform lengths, else FFD_ERR_UNSUPPORTED. */
enum { FFD_FRESCA_SPATIAL = 0, FFD_FRESCA_ENERGY = 1 };
int ffd_fresca(const float* in, float* out, float* work, int B, int L, int C, float low_scale, float high_scale,
               double cutoff_ratio, int strategy, void* stream);

/* The 4-D branch of frequency_scale (fresca.py:184-213): in / out (B, H, W, C), rfft2 / irfft2 over (H, W), ortho;
 * low-pass mask [sqrt(kh^2 + kw^2) <= Rc] on the raw bin indices of the (H, W/2+1) half spectrum (fresca.py:73-81);
 * "spatial": Rc = cutoff_ratio * min(H/2, (W/2+1)/2); "energy": the first integer radius R in 0..int(min(H, W/2+1)/2)
 * whose disc holds cutoff_ratio of the batch-and-channel mean |X| (fresca.py:89-101), 0 if none does.  Not on the
 * sampling path (scores are 3-D); H, W <= 256 and H*W <= 4096, else FFD_ERR_UNSUPPORTED.
 * `work` = 3*B*C*H*(W/2+1) + 4 floats of scratch (8-byte aligned).  Context-free; in != out. */
int ffd_fresca2d(const float* in, float* out, float* work, int B, int H, int W, int C, float low_scale,
                 float high_scale, double cutoff_ratio, int strategy, void* stream);

/* DiffusionSampler(use_fresca=True, ...) (sampler.py:21-26,79-93): apply FreSca to every score
 * inside ffd_sample_batch, with the reference's time-dependent high scale
 * h(t) = (1 - t/num_steps)*(h-1) + 1 for h > 1 (fresca.py:247-257; num_steps <= 0: static h). */
typedef struct {
  float low_scale, high_scale;
  double cutoff_ratio;
  int32_t strategy;   /* FFD_FRESCA_* */
  int32_t num_steps;  /* the sampler's _num_diffusion_steps, or 0 when unset */
} ffd_fresca_cfg;
int ffd_fresca_enable(ffd_ctx* ctx, const ffd_fresca_cfg* cfg);
int ffd_fresca_disable(ffd_ctx* ctx);

/* ---- FreqCa helpers (E2CRFCache(use_freqca=True), caching.py:486-522,561-597) ---- */

/* frequency_decompose_fft / frequency_decompose_dct (fourier.py:219-286; the dct variant returns the
 * fft result, fourier.py:303): low = irfft(rfft(x)[k < n_low]), high = irfft(rfft(x)[k >= n_low]) along
 * dim 1 of x (B, L, D), n_low = max(1, int((L/2+1) * low_freq_ratio)), ortho norm.  low/high must not
 * alias x.  2 <= L <= 4096 within the supported transform lengths, else FFD_ERR_UNSUPPORTED. */
int ffd_freq_decompose(const float* x, float* low, float* high, int B, int L, int D, double low_freq_ratio,
                       void* stream);

/* predict_hermite (fourier.py:397-497): least-squares fit of Hermite polynomials H_0..H_order over the K
 * history points (timesteps normalised to [-1,1], ridge 1e-6) evaluated at `target`.
 * history: device (K, n) stacked tensors; timesteps: host K doubles; out: device n floats.
 * K < 2 or equal timesteps return history[K-1] (fourier.py:416-428).  K <= 32, order <= 8. */
int ffd_hermite_predict(const float* history, const double* timesteps, double target, int order, float* out, int K,
                        size_t n, void* stream);

/* spectral_density (fourier.py:97-131) of a PACKED spectrum xf (B, L, C) -> out (B, L/2+1, C);
 * callers with time-domain input run ffd_dft first (apply_dft=True). */
int ffd_spectral_density(const float* xf, float* out, int B, int L, int C, void* stream);

/* ---- localization metrics, frequency smoothing, spectral profiles (src/fdiff/utils/fourier.py:134-216,
 * src/fdiff/visualization/spectral_interpretation.py:55-94) ----
 * x: time-domain series, dense fp32 (B, L, C) on the device.  Context-free, stream ordered, no host synchronisation, no
 * atomics; every reduction is a fixed-order fp64 tree (inside the matrix product: the fixed chain over t), so results
 * are bit-identical from run to run and a sample's values do not depend on the other samples of the call.  `work`:
 * device scratch of at least the matching *_work_bytes (0 for shapes the call refuses), 8-byte aligned.
 * FFD_ERR_INVALID: a null pointer, B, L, C < 1, work_bytes too small (checked before any device work);
 * FFD_ERR_UNSUPPORTED: L outside the supported transform lengths (L > 8192, or 6826 < L < 8192), B > 2^24, C > 2^16;
 * also checked before any device work. */

/* localization_metrics (fourier.py:134-182): per sample the delocalization min_s sum_t p[t] cyc(t, s)^2,
 * cyc(t, s) = min(|t - s|, L - |t - s|), of p = the energy over time normalized to 1 (deloc_time_out, B floats) and of
 * p = the spectral density mirrored to the full length-L frequency axis (fourier.py:154-159) normalized to 1
 * (deloc_freq_out, B floats).  The (B, L) x (L, L) products run on the fp32 matrix cores with cyc^2 (exact in fp32)
 * made in registers; the minimum is taken in the epilogue.  An all-zero sample gives NaN (0 / 0) in both; L = 1 gives 0. */
size_t ffd_localization_work_bytes(int B, int L, int C);
int ffd_localization(const float* x, float* deloc_time_out, float* deloc_freq_out, void* work, size_t work_bytes, int B,
                     int L, int C, void* stream);
/* smooth_frequency (fourier.py:185-216): out = idft(dft(x) contracted over the packed axis with the column-normalized
 * Gaussian kernel W[t, s] = exp(-((k_t - k_s) / sigma)^2 / 2) / sum_t (...), k = [0 .. (L-1)/2, 1 .. (L-1)/2]).  W is
 * built once per call into `work`; the contraction runs on the fp32 matrix cores.  The reference's k has length L only
 * for odd L (its einsum raises otherwise): even L, sigma <= 0 or non-finite, x == out are FFD_ERR_INVALID; L > 2047 is
 * FFD_ERR_UNSUPPORTED (work_bytes: 0 for both).  L = 1 is the identity. */
size_t ffd_smooth_frequency_work_bytes(int B, int L, int C);
int ffd_smooth_frequency(const float* x, float* out, void* work, size_t work_bytes, int B, int L, int C, double sigma,
                         void* stream);
/* The curves of process_dataset (spectral_interpretation.py:55-94): with d[b, k] = sum_c |X_k|^2 over the L/2 + 1
 * density bins and e[b, t] = sum_c x^2,
 *   spec_mean[k]   = mean_b d / (EPS + sum_k d)     spec_se[k]    = std_b (d / sum_k d) / sqrt(B)      (L/2 + 1 floats each)
 *   energy_mean[t] = mean_b e / (EPS + sum_t e)     energy_std[t] = std_b (e / sum_t e)                (L floats each)
 * EPS = 1e-15, std unbiased (B = 1: NaN, like torch.std); the temporal "SE" column of the reference is the plain std.
 * Two passes over fixed slabs of 1024 samples in fp64. */
size_t ffd_spectral_profile_work_bytes(int B, int L, int C);
int ffd_spectral_profile(const float* x, float* spec_mean, float* spec_se, float* energy_mean, float* energy_std,
                         void* work, size_t work_bytes, int B, int L, int C, void* stream);
/* The longest row (L) whose 32-row block the product kernel of ffd_localization keeps in LDS; above it the rows are
 * read from L2 per centre tile (same results, a slower path).  Host only. */
int ffd_localization_lds_max_len(void);
/* Benchmark helper (replaces nothing in the reference; tools/spectral_bench.py): the stages of ffd_localization with HIP
 * events between them, `warmup` untimed and `iters` timed runs.  x holds n_inputs consecutive (B, L, C) inputs, run i
 * reads input i % n_inputs.  ms_out[3 i + 0..2] = mean, minimum, maximum milliseconds of stage i: the time-domain rows,
 * dft + density + frequency rows, the two product launches.  Synchronous. */
int ffd_localization_bench(const float* x, int n_inputs, float* deloc_time_out, float* deloc_freq_out, void* work,
                           size_t work_bytes, int B, int L, int C, int warmup, int iters, float* ms_out, void* stream);

/* ---- sample metrics: sliced / marginal Wasserstein-2 distances (src/fdiff/utils/wasserstein.py) ----
 * For one direction u the two sets are projected (fp32, exact-fp32 MFMA), each projection is sorted, and
 *   W2^2 = integral over t in [0,1] of (a[floor(t n)] - b[floor(t m)])^2
 * is summed in fp64 over the intervals of the integer grid n*m: what ot.emd2_1d returns for uniform weights
 * (wasserstein.py:116-117,142-143).  standardise != 0 divides by the population std of orig's projection
 * (wasserstein.py:152-160).  orig (n, D), other (m, D), dirs (K, D): fp32 device, dense row-major (float64 data is
 * rounded to fp32 by the caller); dist_out: K doubles on the device.  Reductions are fixed-order fp64 trees without
 * atomics: results are bit-identical from run to run and do not depend on work_bytes.  NaN input: unspecified.
 * Context-free, stream ordered, no host synchronisation.  `work`: device scratch of
 * ffd_w2_work_bytes(n, m, D, K, budget) bytes = kb * 4 * (n + m + max(n, m)), kb = the directions handled at once
 * (as many as `budget_bytes` allows, at least 1, at most K): a smaller buffer means more blocks, never other results.
 * FFD_ERR_INVALID: n, m, D, K < 1, a null pointer, or work_bytes below one direction's need;
 * FFD_ERR_UNSUPPORTED: n, m > 2^26 or D, K > 2^20. */
size_t ffd_w2_work_bytes(int n, int m, int D, int K, size_t budget_bytes);
/* WassersteinDistances.sliced_distances / directional_distance (wasserstein.py:120-144,162-181):
 * dist_out[k] = W2(orig . dirs[k], other . dirs[k]). */
int ffd_w2_sliced(const float* orig, int n, const float* other, int m, int D, const float* dirs, int K,
                  int standardise, double* dist_out, void* work, size_t work_bytes, void* stream);
/* WassersteinDistances.marginal_distances / feature_distance (wasserstein.py:95-118,183-199): K = D, direction k is
 * the k-th basis vector, i.e. column k (a transpose instead of a product). */
int ffd_w2_marginal(const float* orig, int n, const float* other, int m, int D, int standardise, double* dist_out,
                    void* work, size_t work_bytes, void* stream);
/* The same in two steps, so that a Metric object (metrics.py:100-217, which re-creates its directions from one seed at
 * every call, metrics.py:113-119) projects and sorts its original set once: prepared_out (K, n) fp32 = row k holds
 * the ascending projections of x (n, D) on dirs[k] (dirs == NULL: K == D, row k = sorted column k; -0.0 sorts before
 * +0.0).  work: ffd_w2_work_bytes(n, 0, D, K, budget) = kb * 4 * n bytes. */
int ffd_w2_prepare(const float* x, int n, int D, const float* dirs, int K, float* prepared_out, void* work,
                   size_t work_bytes, void* stream);
/* dist_out[k] = W2(prepared row k, other . dirs[k]) with the dirs ffd_w2_prepare was given.
 * work: ffd_w2_work_bytes(0, m, D, K, budget) = kb * 8 * m bytes. */
int ffd_w2_against_prepared(const float* prepared, int n, const float* other, int m, int D, const float* dirs, int K,
                            int standardise, double* dist_out, void* work, size_t work_bytes, void* stream);
/* np.mean / np.max of the distances (metrics.py:120-123,179-182): mean_max_out[0] = mean, [1] = max (device doubles). */
int ffd_w2_summary(const double* dist, int K, double* mean_max_out, void* stream);
/* np.mean(original_samples, axis=0) of the "dummy" baseline (metrics.py:140,199): mean_out (D) fp32, summed in fp64
 * over fixed slabs of 1024 rows in a fixed order (n <= 2^25).  work: ffd_col_mean_work_bytes(n, D) bytes, 8-byte aligned. */
size_t ffd_col_mean_work_bytes(int n, int D);
int ffd_col_mean(const float* x, int n, int D, float* mean_out, void* work, size_t work_bytes, void* stream);

/* Benchmark helper for the kernels above (replaces nothing in the reference; tools/metrics_bench.py): `iters` times,
 * after one warm-up, project x (n, D) on dirs (K, D) into rows (K, n), sort them (scratch: K * n floats), integrate
 * against other_rows (K, m, sorted) into dist (K), and transpose columns [0, min(K, D)) of x into scratch (K <= 32768).
 * ms_out[0..3] = mean milliseconds of the projection, the sort, the integral, the column transpose.  Synchronous. */
int ffd_w2_bench_kernels(const float* x, int n, int D, const float* dirs, int K, float* rows, float* scratch,
                         const float* other_rows, int m, double* dist, int iters, float* ms_out, void* stream);

/* ---- scores of a forecast / imputation ensemble against the truth (an extension beyond the reference) ----
 * ens (S, m, D): S series, m members each, D = L * C coordinates as the samplers return them; truth (S, D);
 * weight NULL (all ones) or (weight_batch, D) with weight_batch 1 (shared) or S, entries 0 or 1: a coordinate with
 * weight 0 (an observed one) is excluded from every score and its per-point outputs are written as 0.  All fp32 on the
 * device, dense row-major.  With x_(1) <= ... <= x_(m) the sorted members of one point and y its truth:
 *   crps[s,d]     = (1/m) sum_i |x_i - y| - (1/Z) sum_i (2 i - m - 1) x_(i);  Z = m^2, or m (m - 1) with fair != 0
 *                   (Ferro's unbiased estimator, needs m >= 2)
 *   crps_mean[s]  = the mean of crps[s,:] over the coordinates with weight 1 (0 if there is none)
 *   quant[q,s,d]  = numpy's default (type 7, linear) quantile of the m members at level levels[q] in [0, 1]: with
 *                   h = (m - 1) p the value x_(floor(h)+1) + (h - floor(h)) (x_(floor(h)+2) - x_(floor(h)+1)), in fp64 with
 *                   numpy's own rounding order (levels 0 and 1: the minimum and maximum themselves); 1 <= n_q <= 64
 *   below, equal  = the number of members < y and == y (the caller forms rank / PIT and coverage from them)
 *   energy[s]     = (1/m) sum_i ||x_i - y||_w - (1/(2Z)) sum_i sum_j ||x_i - x_j||_w,  ||v||_w = sqrt(sum_d w_d v_d^2)
 * crps, below, equal: (S, D); quant: (n_q, S, D); crps_mean, energy: (S); doubles / int32 on the device.  `levels` is a
 * HOST array of n_q doubles.  Any output pointer of ffd_ens_pointwise may be NULL: that output is skipped.
 * Per point: the tiled transpose and the segmented sort of the Wasserstein metrics, then one kernel that reads a sorted
 * row once.  Energy: the pair term from the Gram matrix (exact-fp32 MFMA) of the rows centred on the series' ensemble
 * mean -- uncentred it cancels for a tight ensemble far from the origin -- the truth term in difference form in fp64.
 * Every reduction is a fixed-order fp64 tree without atomics and every tiling depends on (m, D) alone: a series' outputs
 * depend on its own data only, are bit-identical from run to run, for a series scored alone or inside a batch, and for
 * every work_bytes.  NaN input: unspecified.  Context-free, stream ordered, no host synchronisation.
 * `work`: device scratch, 16-byte aligned, of ffd_ens_work_bytes(S, m, D, n_q, budget) bytes, which serves both calls:
 * the larger of 8 S D + 8 m rb (rb = the rows (s, d) sorted at once) and sb * (the energy score's need per series: about
 * 4 m (16 ceil(D / 16) + 3) bytes), with rb, sb as large as `budget_bytes` allows, at least 1: a smaller buffer means more
 * blocks, never other results.  0 for arguments the calls refuse.
 * FFD_ERR_INVALID before any device work: a null pointer (weight and skipped outputs excepted), S, m, D < 1, fair with
 * m < 2, a level outside [0, 1], n_q > 64, weight_batch not 1 or S, work_bytes below one block's need;
 * FFD_ERR_UNSUPPORTED: S, m or D > 2^20. */
size_t ffd_ens_work_bytes(int S, int m, int D, int n_q, size_t budget_bytes);
int ffd_ens_pointwise(const float* ens, const float* truth, const float* weight, int weight_batch, int S, int m, int D,
                      const double* levels, int n_q, int fair, double* crps_out, double* crps_mean_out, double* quant_out,
                      int* below_out, int* equal_out, void* work, size_t work_bytes, void* stream);
int ffd_ens_energy(const float* ens, const float* truth, const float* weight, int weight_batch, int S, int m, int D, int fair,
                   double* energy_out, void* work, size_t work_bytes, void* stream);
/* Benchmark helper (tools/ensemble_bench.py): ffd_ens_energy with HIP events between its stages, `iters` times after one
 * warm-up; the workspace must take all S series in one block (FFD_ERR_INVALID otherwise).  ms_out[0] = mean milliseconds
 * of the ensemble mean + centring + truth term, ms_out[1] = of the pair kernel.  Synchronous. */
int ffd_ens_bench_energy(const float* ens, const float* truth, const float* weight, int weight_batch, int S, int m, int D,
                         int fair, double* energy_out, void* work, size_t work_bytes, int iters, float* ms_out,
                         void* stream);

/* ---- nearest-neighbour statistics between two row sets: k-NN search, ball counts, precision / recall / density /
 * coverage / authenticity (csrc/ffd_neighbours.hip; Kynkaanniemi et al. 2019, Naeem et al. 2020, Alaa et al. 2022) ----
 * query (nq, D) and ref (nr, D): flat fp32 rows on the device, dense row-major, read only.  Distances are squared
 * Euclidean.  Both sets are centred on the reference set's column mean (fixed-order fp64) into the workspace and the
 * pair distances d2(i, j) = (n_i + n_j) - 2 z_i . z_j come from the exact-fp32 MFMA in 64 x 256 tiles, clamped at 0;
 * uncentred, the Gram form loses the distances between neighbours of a cluster away from the origin.
 *   search      per query row the k smallest (d2, index) over all reference rows, ordered by (value, then lower index);
 *               the k kept pairs are then recomputed in difference form in fp64 on the caller's own rows,
 *               sum_d ((double)a_d - (double)b_d)^2 in a fixed order, and sorted again by (value, index): dist2_out
 *               (nq, k) doubles ascending (exactly 0.0 for identical rows), index_out (nq, k) int32.
 *   ball count  count_out[i] = #{ j : d2(i, j) <= radius2[j] } on the same tiles, radius2 (nr) floats; integer partial
 *               counts per (row, column chunk), added in chunk order.
 *   exclude_self != 0 skips the pair i == j; legal only when query and ref are the same buffer and nq == nr.
 * A block of the distance matrix goes through the workspace and one wave per row merges it into the row's running
 * list.  (value, index) is a strict order and an element's bits do not depend on its tile, so the results are
 * bit-identical from run to run, for every work_bytes, and for a query set searched whole or in parts.  No atomics.
 * NaN input: unspecified.  Context-free, stream ordered, no host synchronisation.
 * `work`: device scratch, 16-byte aligned, of at least the bytes the size query returns for (nq, nr, D, k, budget): both
 * centred copies (4 (nq + nr) 16 ceil(D / 16) bytes), norms, mean, the running lists, and a distance block of as many
 * 64 x 256 tiles (a power of two, at least one) as `budget_bytes` holds; the ball count needs what k = 1, budget 0 says.
 * 0 for arguments the calls refuse.
 * FFD_ERR_INVALID before any device work, outputs untouched: a null pointer, nq, nr, D < 1, k < 1 or k > FFD_NN_MAX_K,
 * k > nr - (exclude_self != 0), exclude_self with query != ref or nq != nr, a workspace that is too small or not
 * 16-byte aligned, an output or the workspace overlapping an input or another output;
 * FFD_ERR_UNSUPPORTED: nq or nr > 2^24, D > 2^16. */
enum { FFD_NN_MAX_K = 32 };
size_t ffd_nn_work_bytes(int nq, int nr, int D, int k, size_t budget_bytes);
int ffd_nn_search(const float* query, int nq, const float* ref, int nr, int D, int k, int exclude_self, double* dist2_out,
                  int32_t* index_out, void* work, size_t work_bytes, void* stream);
int ffd_nn_ball_count(const float* query, int nq, const float* ref, int nr, int D, const float* radius2, int exclude_self,
                      int32_t* count_out, void* work, size_t work_bytes, void* stream);
/* radius2_out[i] = (float)dist2[i][col] of a (n, k) search result: the radii of a ball count (0 <= col < k). */
int ffd_nn_radius(const double* dist2, int n, int k, int col, float* radius2_out, void* stream);
/* The eight sample-quality numbers of n originals Y and m samples X from six arrays on the device:
 *   self_dist2 (n, k)   Y searched in itself with exclude_self: column 0 is r_1(y)^2, column k - 1 is r_k(y)^2
 *   xy_dist2, xy_index (m)   each sample's nearest original;  yx_dist2 (n)   each original's nearest sample
 *   count_x (m) = #{ y : d(x, y) <= r_k(y) };  count_y (n) = #{ x : d(y, x) <= rho_k(x) }, rho_k inside X
 * out8 = precision (share of x with count_x > 0), recall (share of y with count_y > 0), density (sum count_x / (k m)),
 * coverage (share of y with yx_dist2 <= r_k(y)^2), authenticity (share of x with xy_dist2 > r_1(y*)^2, y* = xy_index),
 * the mean and the minimum over x of sqrt(xy_dist2), and the share of x with xy_dist2 == 0; fixed-order fp64 sums.
 * FFD_ERR_INVALID: a null pointer, n, m < 1, k outside [1, FFD_NN_MAX_K], out8 overlapping an input. */
int ffd_nn_scores(const double* self_dist2, const double* xy_dist2, const int32_t* xy_index, const double* yx_dist2,
                  const int32_t* count_x, const int32_t* count_y, int n, int m, int k, double* out8, void* stream);

/* ---- kernel two-sample statistics: Gaussian-kernel row sums, MMD^2, witness values, a bandwidth and a permutation test
 * (csrc/ffd_mmd.hip; Gretton et al. 2012) ----
 * k_gamma(a, b) = exp(-gamma |a - b|^2); `gammas`: a HOST array of n_gamma doubles, 1 <= n_gamma <= FFD_MMD_MAX_GAMMAS,
 * each finite and >= 0.  Row sets are flat fp32 rows on the device, dense row-major, read only.  Both sets of a call
 * are centred on ONE caller-supplied vector `centre` (D floats on the device; ffd_mmd_centre computes a set's column
 * mean with the nearest-neighbour kernels' fixed-order fp64 mean) and d2 comes from the same Gram statement as ffd_nn_*:
 * exact-fp32 MFMA in 64 x 256 tiles, (n_i + n_j) - 2 z_i . z_j clamped at 0.  Kernel values are fp32 (one hardware
 * exponential per gamma and pair; a doubling ladder is not special-cased) and are added in fp64.
 *   row sums    rowsum_out[g][i] = sum_j k_gamma_g(a_i, b_j) over all rows of b, (n_gamma, na) doubles.  exclude_self != 0
 *               skips the pair i == j (never computed and subtracted); legal only when a and b are the same buffer and
 *               na == nb.  A workgroup owns 64 query rows and walks a run of 4 column tiles (1024 columns; a constant of
 *               the source) in order; the runs' partial sums are folded in run order.  So a row's sum depends on the
 *               row, the column set, the centre and the gammas alone: bit-identical from run to run, for a query set
 *               summed whole or in parts, whatever rows surround it, and for n_gamma gammas at once or one at a time.
 *               gamma = 0 gives exactly the column count.  No distance block goes through memory.
 *               For D > 1024 the tile's sum over the coordinates is taken in chunks of 1024 (partial sums kept in LDS and
 *               added in order): a single fp32 chain over 65 536 terms would miss the accuracy below on kernel values.
 *   bandwidth   sigma2_out[0] = 2 (n / (n - 1)) mean_j |y_j - ybar|^2, the mean squared distance between two distinct rows,
 *               from the fp64 column mean and fp64 squared deviations in a fixed order; no pair is formed.  n >= 2.
 *   scores      from the three row-sum arrays XX (n_gamma, n; self excluded), XY (n_gamma, n) and YY (n_gamma, m; self
 *               excluded) of n samples X and m originals Y: mmd2_out (2, n_gamma + 1) doubles, row 0 the unbiased
 *               sum xx / (n (n - 1)) + sum yy / (m (m - 1)) - 2 sum xy / (n m), row 1 the biased one (exactly 1 per row
 *               added for the diagonal, divided by n^2 and m^2); column g that gamma, column n_gamma the mean kernel over
 *               the gammas.  witness_out[i] = xx[i] / (n - 1) - xy[i] / m for the mean kernel, n doubles.  n, m >= 2.
 *               The sums run in ONE workgroup (a fixed-order tree), so the call streams 8 n_gamma (2 n + m) bytes
 *               through one compute unit: sized for evaluation sets (4.3 MB at 10 000 x 87 554 rows and 5 gammas);
 *               at the row limit with 8 gammas it is 3 GB and takes accordingly.
 *   gram        the pooled mean-kernel matrix K of the N = n + m rows (x first), N rows of 64 ceil(N / 64) floats, diagonal
 *               0, at the start of `work`.
 *   permute     T_p = a^T K a / (n (n - 1)) + b^T K b / (m (m - 1)) - 2 a^T K b / (n m) for P assignments: `assign` (P, N)
 *               uint8 on the device with exactly n nonzero entries per row (the caller's to guarantee), b = 1 - a;
 *               `gram_work` is the workspace ffd_mmd_gram filled.  K A^T runs on the fp64 matrix instruction, where K's
 *               fp32 entries and the assignments are exact; t_out (P) doubles, fixed-order sums.  The assignment
 *               (1, ..., 1, 0, ..., 0) gives the unbiased MMD^2 of the mean kernel.
 * Context-free, stream ordered, no host synchronisation, no atomics.  NaN input: unspecified.
 * `work`: device scratch, 16-byte aligned, of at least the bytes the matching size query returns; 0 for arguments the
 * call refuses.
 * FFD_ERR_INVALID before any device work, outputs untouched: a null pointer, a count < 1 (n, m < 2 for bandwidth, scores,
 * gram and permute), n_gamma outside [1, 8], a gamma that is negative, not finite or too large for fp32, exclude_self
 * with a != b or na != nb, a workspace that is too small or not 16-byte aligned, an output or the workspace overlapping
 * an input or another output;
 * FFD_ERR_UNSUPPORTED: rows > 2^24, D > 2^16, n + m > FFD_MMD_MAX_POOLED, P > FFD_MMD_MAX_PERMUTATIONS. */
enum { FFD_MMD_MAX_GAMMAS = 8, FFD_MMD_MAX_POOLED = 16384, FFD_MMD_MAX_PERMUTATIONS = 4096 };
size_t ffd_mmd_centre_work_bytes(int n, int D);
int ffd_mmd_centre(const float* x, int n, int D, float* centre_out, void* work, size_t work_bytes, void* stream);
size_t ffd_mmd_bandwidth_work_bytes(int n, int D);
int ffd_mmd_bandwidth(const float* y, int n, int D, double* sigma2_out, void* work, size_t work_bytes, void* stream);
size_t ffd_mmd_rowsums_work_bytes(int na, int nb, int D, int n_gamma);
int ffd_mmd_rowsums(const float* a, int na, const float* b, int nb, int D, const float* centre, const double* gammas,
                    int n_gamma, int exclude_self, double* rowsum_out, void* work, size_t work_bytes, void* stream);
int ffd_mmd_scores(const double* rowsum_xx, const double* rowsum_xy, const double* rowsum_yy, int n, int m, int n_gamma,
                   double* mmd2_out, double* witness_out, void* stream);
size_t ffd_mmd_gram_work_bytes(int n, int m, int D);
int ffd_mmd_gram(const float* x, int n, const float* y, int m, int D, const float* centre, const double* gammas, int n_gamma,
                 void* work, size_t work_bytes, void* stream);
size_t ffd_mmd_permute_work_bytes(int n, int m, int P);
int ffd_mmd_permute(const void* gram_work, int n, int m, const uint8_t* assign, int P, double* t_out, void* work,
                    size_t work_bytes, void* stream);

/* ---- entropic optimal transport between two row sets: the softmin of the squared-distance cost, the symmetric Sinkhorn
 * loop and the Sinkhorn divergence (csrc/ffd_sinkhorn.hip; Cuturi 2013; Genevay, Peyre, Cuturi 2018; Feydy et al. 2019) ----
 * Row sets are flat fp32 rows on the device, dense row-major, read only, with uniform weights.  Both sets of a call are
 * centred on ONE caller-supplied vector `centre` (D floats on the device, ffd_mmd_centre) and C_ij = |x_i - y_j|^2 comes
 * from the same Gram statement as ffd_nn_* and ffd_mmd_*: exact-fp32 MFMA in 64 x 256 tiles, (n_i + n_j) - 2 z_i . z_j
 * clamped at 0, in chunks of 1024 coordinates for D > 1024.  Potentials are doubles on the device.
 *   softmin   out[i] = -eps log( (1 / nr) sum_j exp((h[j] - C_ij) / eps) ), nq doubles; with `old` (nq doubles, may be
 *             NULL) the damped update out[i] = (old[i] + that) / 2.  h is rounded once to fp32; the exponent and the
 *             exponential are fp32 (one hardware exponential per pair; a term within 2^(-1/8) of the row's maximum is
 *             1 + (2^t - 1) with the difference from its series, so that a large eps, where every term is 1 - x, keeps
 *             x), a row's running (max, sum) keeps its sum in fp64.
 *             A workgroup owns 64 query rows and walks a run of 4 column tiles (1024 columns; a constant of the source)
 *             in order; the lanes', waves' and runs' (max, sum) pairs are merged in fp64 in a fixed order.  So out[i]
 *             depends on the row, the column set, h, the centre and eps alone: bit-identical from run to run, for a
 *             query set cut in parts, whatever rows surround it.  No cost block goes through memory.
 *   loop      the symmetric, Jacobi-ordered iteration over `eps_schedule` (a HOST array of n_eps doubles): all potentials
 *             start at 0 and in pass e every one is updated from the values of pass e - 1 alone,
 *               f <- (f + softmin(x | y, g)) / 2     g <- (g + softmin(y | x, f)) / 2
 *               p <- (p + softmin(x | x, p)) / 2     q <- (q + softmin(y | y, q)) / 2
 *             (pass 0: the softmin itself), then one undamped pass at the last eps from the last damped values writes
 *             f_out, p_out (n doubles) and g_out, q_out (m doubles).  out3 = { S = mean (f - p) + mean (g - q),
 *             OT_eps(x, y) = mean f + mean g, the largest |change| of f and g in the last damped pass }: fixed-order fp64.
 *             For two sets of equal rows the x|y and x|x problems are the same computation: S is exactly 0.0.
 *             q_in (m doubles on the device, or NULL): an already converged self potential of y; the y|y passes are
 *             skipped and q_out is its copy.  q does not depend on x: the q_out of any call on the same y, centre and
 *             schedule may be handed to the next.
 *   diameter  diameter2_out[0] = 4 max_j |y_j - centre|^2 (one double on the device): the square of twice the largest
 *             radius about the centre, an upper bound of every squared distance inside the set; the fp32 differences
 *             the tile is built from, squared and added in fp64.  Where a schedule starts.
 *   schedule  ffd_host_sinkhorn_schedule, host only: diameter2, diameter2 scaling^2, diameter2 scaling^4, ... while the
 *             value is above eps_target, then n_final entries of eps_target.  Returns the count; when it exceeds
 *             `capacity` nothing is written (out may then be NULL).  FFD_ERR_INVALID: diameter2 or eps_target not finite
 *             or <= 0, scaling outside (0, 1), n_final < 1, capacity < 0; FFD_ERR_UNSUPPORTED: more than 2^20 entries.
 * Context-free, stream ordered, no host synchronisation, no atomics, no cross-workgroup waiting.  NaN input: unspecified.
 * `work`: device scratch, 16-byte aligned, of at least the bytes the matching size query returns; 0 for arguments the
 * call refuses.
 * FFD_ERR_INVALID before any device work, outputs untouched: a null pointer (old and q_in excepted), a count < 1, n_eps
 * < 1, an eps that is not finite, is <= 0 or whose log2(e) / eps is no normal fp32 number, a workspace that is too small
 * or not 16-byte aligned, an output or the workspace overlapping an input or another output;
 * FFD_ERR_UNSUPPORTED: rows > 2^24, D > 2^16. */
size_t ffd_sinkhorn_softmin_work_bytes(int nq, int nr, int D);
int ffd_sinkhorn_softmin(const float* query, int nq, const float* ref, int nr, int D, const float* centre, const double* h,
                         double eps, const double* old, double* out, void* work, size_t work_bytes, void* stream);
size_t ffd_sinkhorn_work_bytes(int n, int m, int D);
int ffd_sinkhorn(const float* x, int n, const float* y, int m, int D, const float* centre, const double* eps_schedule,
                 int n_eps, const double* q_in, double* f_out, double* g_out, double* p_out, double* q_out, double* out3,
                 void* work, size_t work_bytes, void* stream);
size_t ffd_sinkhorn_diameter2_work_bytes(int n, int D);
int ffd_sinkhorn_diameter2(const float* y, int n, int D, const float* centre, double* diameter2_out, void* work,
                           size_t work_bytes, void* stream);
int ffd_host_sinkhorn_schedule(double diameter2, double eps_target, double scaling, int n_final, double* out, int capacity);

/* ---- the first two moments of a row set in float64: covariance, a symmetric eigensolver, the symmetric square root, the
 * Frechet distance between two fitted Gaussians and principal components (csrc/ffd_pca.hip; Dowson & Landau 1982; Heusel
 * et al. 2017; Golub & Van Loan, Matrix Computations, 8.5) ----
 * Row sets are flat fp32 rows (n, D) on the device, dense row-major, read only.  Everything else is float64 on the device,
 * matrices dense row-major (D, D), and all arithmetic is float64; matrix products run on v_mfma_f64_16x16x4_f64 with k
 * ascending.  1 <= D <= FFD_PCA_MAX_D, 2 <= n <= 2^24 (ffd_pca_transform: n >= 1).
 *   cov        mean_out[d] = the column mean (fixed-order fp64 tree over slabs of 1024 rows); cov_out = D^T D / (n - 1) of
 *              the deviations (double)x - mean, over slabs of 256 rows each summed from zero, the slabs of a run (a count
 *              that depends on n alone; at most 64 runs) added in slab order and the runs in run order.  Only the upper
 *              triangle's 64 x 64 tiles are formed and entry (j, i) is entry (i, j): bitwise symmetric, bit-identical from
 *              run to run.
 *   sym_eig    all eigenvalues of the symmetric matrix `a` (its upper triangle is read; it may be indefinite), ascending in
 *              w_out (D), and with v_out (D, D; may be NULL: then no vectors are accumulated and w_out has the same bits)
 *              the eigenvectors as columns, v_out[d][i] component d of the vector of w_out[i].  Cyclic Jacobi in the
 *              round-robin order: D - 1 rounds (D for odd D, one index sitting out) of floor(D / 2) disjoint rotations, a
 *              round two launches.  For a pair p < q with a_pq != 0: tau = (a_qq - a_pp) / (2 a_pq),
 *              t = sign(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c; a_pq == 0 is skipped.  A sweep
 *              starts only while off(A) > 2^-53 |A|_F; every threshold is relative, so a matrix times a power of two gives
 *              that power times the same eigenvalues and the same vectors, bit for bit.  The matrix stays bitwise symmetric
 *              throughout.  max_sweeps caps the sweeps (0: the default, 30).  info3_host: THREE DOUBLES ON THE HOST =
 *              { sweeps done, the final off(A) / |A|_F, 1.0 if that is <= 2^-53 else 0.0 }: a cap that was hit is FFD_OK
 *              with info3_host[2] = 0.  The test is one 8-byte read-back per sweep: THIS ENTRY SYNCHRONISES ITS STREAM (so
 *              does ffd_frechet) and cannot be captured in a graph.
 *   sym_root   root_out = V diag(sqrt(max(w, 0))) V^T from eigenvalues w (D) and eigenvectors v (D, D, columns); the upper
 *              triangle mirrored: bitwise symmetric.
 *   frechet    out5 (five doubles on the device) = { FD, |mean_x - mean_y|^2, tr S_x + tr S_y - 2 sum_i sqrt(max(l_i, 0)),
 *              tr S_x, tr S_y }, FD the sum of the two terms, l the eigenvalues of M = (P + P^T) / 2, P = R S_x R from two
 *              products, R = root_y or, when root_y is NULL, the sym_root of sym_eig(cov_y); sums are fixed-order trees.
 *              info3_host as for sym_eig, the worst of the decompositions the call made.
 *   variances  out[i] = v_i^T cov v_i for the k eigenvectors of largest eigenvalue, i = 0 the largest (column D - 1 - i of
 *              v, as sym_eig orders them).
 *   transform  scores_out (n, k) = ((double)x - mean) V[:, D - 1 - j], column j = 0 the axis of largest eigenvalue.
 * Context-free, stream ordered, no atomics, no cross-workgroup waiting.  NaN input: unspecified.
 * `work`: device scratch, 16-byte aligned, of at least the bytes the matching size query returns; the queries are monotone
 * in every argument and 0 for arguments the call refuses.
 * FFD_ERR_INVALID before any device work, outputs untouched: a null pointer (v_out and root_y excepted), n < 2 (transform:
 * n < 1), D < 1, k < 1 or k > D, max_sweeps < 0, a workspace that is too small or not 16-byte aligned, an output or the
 * workspace overlapping an input or another output; FFD_ERR_UNSUPPORTED: n > 2^24, D > FFD_PCA_MAX_D. */
enum { FFD_PCA_MAX_D = 1024 };
size_t ffd_cov_work_bytes(int n, int D);
int ffd_cov(const float* x, int n, int D, double* mean_out, double* cov_out, void* work, size_t work_bytes, void* stream);
size_t ffd_sym_eig_work_bytes(int D);
int ffd_sym_eig(const double* a, int D, int max_sweeps, double* w_out, double* v_out, double* info3_host, void* work,
                size_t work_bytes, void* stream);
size_t ffd_sym_root_work_bytes(int D);
int ffd_sym_root(const double* w, const double* v, int D, double* root_out, void* work, size_t work_bytes, void* stream);
size_t ffd_frechet_work_bytes(int D);
int ffd_frechet(const double* mean_x, const double* cov_x, const double* mean_y, const double* cov_y, const double* root_y,
                int D, int max_sweeps, double* out5, double* info3_host, void* work, size_t work_bytes, void* stream);
size_t ffd_pca_variances_work_bytes(int D, int k);
int ffd_pca_variances(const double* cov, const double* v, int D, int k, double* out, void* work, size_t work_bytes,
                      void* stream);
int ffd_pca_transform(const float* x, int n, int D, const double* mean, const double* v, int k, double* scores_out,
                      void* stream);

/* ---- dynamic time warping between two sets of series: banded DTW search, paired DTW, six sample-quality numbers
 * (csrc/ffd_dtw.hip; Sakoe & Chiba 1978; the 1-NN two-sample accuracy of Lopez-Paz & Oquab 2017) ----
 * A series is (L, C) fp32, dense row-major; a set is (n, L, C) on the device, read only.  For a half-width `window` = w:
 *   c(i, j) = sum_ch (a[i,ch] - b[j,ch])^2, fp32, ch = 0 .. C - 1 in order, the product and the sum rounded separately;
 *   D(0, 0) = c(0, 0), D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)) over the cells with |i - j| <= w,
 *   one fp32 add per cell, every cell outside the band or the grid +inf;  dtw2(a, b; w) = D(L-1, L-1), a SQUARED cost.
 * w = 0 is the squared Euclidean distance, w >= L - 1 unconstrained DTW; a window above L - 1 is clipped to L - 1 first.
 * A cell does not depend on the order of evaluation: dtw2 has the same bits for every tiling, is bitwise symmetric in
 * (a, b), and a copied row reads exactly 0.0.  Outputs are fp32, as the recurrence is.
 *   search   per query row the k smallest (dtw2, index) over all reference rows, ordered by (value, then lower index):
 *            dist2_out (nq, k) floats ascending, index_out (nq, k) int32.  exclude_self != 0 skips the pair i == i; legal
 *            only when query and ref are the same buffer and nq == nr.  A lane owns one pair; a block of the pair matrix
 *            goes through the workspace and the nearest-neighbour merge folds it into the running lists, which are the
 *            outputs themselves.  Bit-identical from run to run, for every work_bytes, for a query set searched whole or
 *            in parts, and whatever reference rows follow.
 *   pairs    dist2_out[i] = dtw2(a[i], b[i]; w), n floats.
 *   scores   from five arrays of n originals Y and m samples X, all fp32 on the device: the k = 1 squared DTW distances
 *            xx_d2 (m; X in X, self excluded), xy_d2 (m; X in Y), yx_d2 (n; Y in X), yy_d2 (n; Y in Y, self excluded) and
 *            xy_e2 (m; X in Y at window 0).  out6 doubles: mean_x sqrt(xy_d2); mean_y sqrt(yx_d2); the warp gain
 *            1 - mean over the x with xy_e2 > 0 of sqrt(xy_d2 / xy_e2) (0.0 when there is none); the share of x with
 *            xx_d2 < xy_d2; the share of y with yy_d2 < yx_d2 (both strict); the mean of the two shares.  One workgroup,
 *            fixed-order fp64 trees.  n, m >= 2.
 * `work`: device scratch, 16-byte aligned, of at least the bytes the size query returns: a distance block of as many
 * 64 x 256 units (a power of two, at least one) as `budget_bytes` holds.  A smaller budget means more launches, never
 * other results.  The size query returns 0 for arguments the search refuses.
 * Context-free, stream ordered, no host synchronisation, no atomics.  NaN input: unspecified.
 * FFD_ERR_INVALID before any device work, outputs untouched: a null pointer, a count, L or C < 1, window < 0, k < 1,
 * k > FFD_DTW_MAX_K or k > nr - (exclude_self != 0), exclude_self with query != ref or nq != nr, a workspace that is too
 * small or not 16-byte aligned, an output or the workspace overlapping an input or another output;
 * FFD_ERR_UNSUPPORTED: rows > 2^24, L > FFD_DTW_MAX_LEN, C > FFD_DTW_MAX_CHANNELS, L C > 65 536, a clipped window above
 * FFD_DTW_MAX_WINDOW. */
enum { FFD_DTW_MAX_WINDOW = 64, FFD_DTW_MAX_LEN = 4096, FFD_DTW_MAX_CHANNELS = 64, FFD_DTW_MAX_K = 32 };
size_t ffd_dtw_work_bytes(int nq, int nr, int L, int C, int window, int k, size_t budget_bytes);
int ffd_dtw_search(const float* query, int nq, const float* ref, int nr, int L, int C, int window, int k, int exclude_self,
                   float* dist2_out, int32_t* index_out, void* work, size_t work_bytes, void* stream);
int ffd_dtw_pairs(const float* a, const float* b, int n, int L, int C, int window, float* dist2_out, void* stream);
int ffd_dtw_scores(const float* xx_d2, const float* xy_d2, const float* yx_d2, const float* yy_d2, const float* xy_e2,
                   int n_original, int m_samples, double* out6, void* stream);

/* ---- denoising score-matching loss: the `val/loss` of ScoreModule.validation_step (src/fdiff/utils/losses.py) ----
 * Per sample b, with std[b,l] = sigma[b] * G[l] and n = L * C (losses.py:68-80, sde.py:106-123,187-210):
 *   x_noisy = mean_coeff[b] * x0 + std[b,l] * z                  r = score + z / std[b,l]
 *   default:               loss_b = reduce(w[b] * r^2),  w[b] = 1 / sum_l (1 / std[b,l]^2)     (losses.py:92-109)
 *   likelihood_weighting:  loss_b = reduce((std[b,l] * r)^2)                                    (losses.py:111-122)
 *   reduce = the mean over the n elements, or 0.5 * the sum when reduce_mean == 0               (losses.py:33-37)
 * mean_coeff, sigma: (B) fp32 on the device, SUPPLIED BY THE CALLER like the timestep grid of ffd_sample_batch --
 * VP: exp(lmc) and sqrt(1 - exp(2 lmc)), VE: 1 and sigma_min (sigma_max / sigma_min)^t.  The reference forms them in
 * fp32 and 1 - exp(2 lmc) is ill-conditioned at small t (one ulp of exp moves sigma by 3e-5 relative at t = 0.01), so a
 * library that recomputed them could not reproduce a reference value.  G: (L) fp32 on the device (ffd_host_noise_scaling).
 * Tensors are dense fp32 (B, L, C); everything is stream ordered without host synchronisation and without atomics; the
 * reductions are fixed-order fp64 trees (fp32 terms), so results are bit-identical from run to run.
 * z (B, L, C) injects the N(0,1) draws; z == NULL draws them on the device: Philox4x32-10 keyed by seed under stream tag
 * 0xFFFFFFFE, counted by the global element index (sample_offset + b) * L * C + i as in ffd_sde_step, so a shard draws
 * what the unsharded call draws, and the loss kernel regenerates what the perturbation drew for the same
 * (seed, sample_offset): no z buffer exists on that path.
 * FFD_ERR_INVALID: a null pointer (z excepted), B, L, C < 1, eps >= T, x0 == x_noisy; checked before any device work. */

/* losses.py:60-63: t_out[b] = u * (T - eps) + eps in fp32, u in [0, 1) from Philox (stream tag 0xFFFFFFFD) counted by
 * the global sample index sample_offset + b. */
int ffd_sm_draw_times(float* t_out, int B, double eps, double T, uint64_t seed, uint64_t sample_offset, void* stream);
/* SDE.marginal_prob + SDE.add_noise on Sigma^{1/2} z (losses.py:68-85, sde.py:66-77). */
int ffd_sm_perturb(const float* x0, float* x_noisy, const float* mean_coeff, const float* sigma, const float* G,
                   const float* z, uint64_t seed, uint64_t sample_offset, int B, int L, int C, void* stream);
/* The weighted squared error and its reduction over the data dimensions (losses.py:92-122): per_sample_out = B doubles
 * on the device.  The batch mean (losses.py:124) is element 0 of ffd_w2_summary over them. */
int ffd_sm_loss(const float* score, const float* sigma, const float* G, const float* z, uint64_t seed,
                uint64_t sample_offset, int likelihood_weighting, int reduce_mean, double* per_sample_out, int B, int L,
                int C, void* stream);
/* loss_fn's body for one batch (losses.py:65-122) on a context: the perturbation into a context workspace, the score
 * network at the per-sample `timesteps` (B, device; the uncached path of ffd_score_forward_ts, every backbone) and the
 * loss, with the context's G table.  Does not touch the E2-CRF cache. */
int ffd_sm_eval_batch(ffd_ctx* ctx, const float* x0, const float* timesteps, const float* mean_coeff, const float* sigma,
                      const float* z, uint64_t seed, uint64_t sample_offset, int likelihood_weighting, int reduce_mean,
                      double* per_sample_out, int B, void* stream);

/* ---- training (csrc/ffd_train.hip): backward pass, gradient norm, AdamW -- score_models.py:290-324 without dropout ----
 * Built for the transformer (FFD_MODEL_TRANSFORMER: head_dim <= 8, max_len <= 512, any d_model, dim_feedforward, C, B)
 * and the MLP backbone (FFD_MODEL_MLP).  The LSTM has no backpropagation through time and the mixture nothing to train:
 * ffd_train_create answers FFD_ERR_UNSUPPORTED for them, as for dropout != 0.
 * The transformer's training forward is a second implementation of the forward from generic pieces (launch_dense, the
 * LayerNorm and attention operators below) that keeps, per layer: the layer input, qkv, the attention output before the
 * out-projection, the normalised LN1 rows, the LN1 output, both LayerNorms' rstd, the post-ReLU hidden activation and each
 * attention row's log-sum-exp.  Its positional table is nn.Embedding(max_norm = sqrt(d_model)): every batch call first
 * renormalises the bound PARAMETER's rows in place (k_renorm_rows, as torch's lookup does without gradient), and the
 * table's gradient sum_b dh0[b, l, :] is taken with respect to the renormalised rows.  The time encoder's dense layer
 * gets dtemb[b, :] = sum_l dh0[b, l, :] against the sin / cos features; time_encoder.W is frozen.
 * Everything is exact fp32 on v_mfma_f32_16x16x4_f32, stream ordered, without atomics and, once the object's
 * workspace and tensor table exist (below), without a host synchronisation; every reduction is a fixed-order tree (fp64 where it adds many fp32 terms): results are bit-identical
 * from run to run.  All argument errors are returned before any device work. */

/* Dense backward, row-major fp32, any M, N, K >= 1 (FFD_ERR_UNSUPPORTED when M N, M K or N K reaches 2^31, or N or K
 * exceeds 65 535 * 64):
 *   dgrad  dX[M,K] = mask(dY[M,N] . W[N,K]) + R    act (M, K) or NULL: the saved post-ReLU activation, dX = 0 where it
 *                                                  is not positive;  R (M, K) or NULL is added after the mask
 *   wgrad  dW[N,K] = dY^T . X[M,K];  db[N] (or NULL) = the column sums of dY in fp64
 * wgrad cuts M into the chunks the query below counts -- a function of the shape alone: at most 1024 rows each, finer
 * (down to 64 rows) where N x K has few 64 x 64 tiles, at most 64 chunks -- runs them as independent workgroups and adds
 * their partial results in chunk order in fp64.  `work` holds the partials: the bytes the query gives (0 for one chunk),
 * 8-byte aligned. */
int ffd_dense_dgrad(const float* dY, const float* W, const float* act, const float* R, float* dX, int M, int N, int K,
                    void* stream);
int ffd_dense_wgrad_chunks(int M, int N, int K);
size_t ffd_dense_wgrad_work_bytes(int M, int N, int K);
int ffd_dense_wgrad(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, void* work,
                    size_t work_bytes, void* stream);

/* The per-sample losses of ffd_sm_loss (reduce_mean = 1, the same bits) together with the gradient of their batch mean:
 *   default:               dscore = 2 w[b] r / (L C B)          likelihood_weighting:  dscore = 2 std[b,l]^2 r / (L C B)
 * z == NULL regenerates the draws of the perturbation under the same stream tag 0xFFFFFFFE, counted by the global sample
 * sample_offset + (index ? index[b] : b); index: (B) int64 on the device or NULL.  score, sigma, z, dscore: batch order. */
int ffd_sm_loss_grad(const float* score, const float* sigma, const float* G, const float* z, uint64_t seed,
                     uint64_t sample_offset, const int64_t* index, int likelihood_weighting, double* per_sample_out,
                     float* dscore, int B, int L, int C, void* stream);

/* The rows index[b] of ffd_sm_draw_times: t_out[b] = the draw of global sample sample_offset + index[b] (index: (B) int64
 * on the device), so a shuffled batch draws B times, not the data set's. */
int ffd_sm_draw_times_at(float* t_out, const int64_t* index, int B, double eps, double T, uint64_t seed,
                         uint64_t sample_offset, void* stream);

/* Operators of the transformer's training forward and backward, callable on their own.  LayerNorm over the last dimension of x (M, D), biased variance: the forward also stores the
 * normalised rows xhat (M, D) and every row's reciprocal deviation rstd (M); the backward takes them,
 *   dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma;  dgamma = sum_m dy xhat, dbeta = sum_m dy (fp64, fixed order).
 * Attention for head_dim <= 8 and L <= 512 (FFD_ERR_UNSUPPORTED beyond) on the in-projection's row-major output
 * qkv (B L, 3 H hd) = q | k | v with head h at columns h hd of each third: out (B L, H hd) = softmax(q k^T / sqrt(hd)) v
 * and lse (B, H, L), each row's log-sum-exp of the scaled scores; the backward recomputes the probabilities from lse and
 * writes dqkv (B L, 3 H hd), every element once (nothing accumulates across workgroups). */
int ffd_layernorm_stats_fwd(const float* x, const float* gamma, const float* beta, float* y, float* xhat, float* rstd,
                            int M, int D, double eps, void* stream);
int ffd_layernorm_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx, float* dgamma,
                      float* dbeta, int M, int D, void* stream);
int ffd_attention_lse_fwd(const float* qkv, float* out, float* lse, int B, int L, int H, int hd, void* stream);
int ffd_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int L,
                      int H, int hd, void* stream);

/* torch.optim.AdamW's arithmetic in its order (decoupled decay, moments, bias corrections, update) at step >= 1 (the
 * count including this step), on the gradient times the clip coefficient min(1, max_norm / (sqrt(*sqnorm) + 1e-6))
 * (torch.nn.utils.clip_grad_norm_).  sqnorm: one double on the device, read by the kernel; NULL or max_norm <= 0: no
 * clipping.  The gradient buffer is not modified (it keeps the unclipped gradient). */
typedef struct {
  double lr, beta1, beta2, eps, weight_decay, max_norm;
  long long step;
} ffd_adamw_cfg;
int ffd_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const double* sqnorm,
              const ffd_adamw_cfg* cfg, void* stream);

/* The learning rate at `step` (host only): lr_max step / max(1, warm-up) below the warm-up, then
 * lr_max max(0, (1 + cos(pi progress)) / 2), progress = (step - warm-up) / max(1, total - warm-up). */
double ffd_host_lr_schedule(double lr_max, long long step, long long num_warmup_steps, long long num_training_steps);

/* The training object.  Separate from ffd_ctx (which keeps packed copies of the weights): it works on the caller's
 * tensors in place -- ffd_train_bind gives the device pointers of one named parameter (the state_dict key), its
 * gradient and the two Adam moments, n elements each; no second set of weights exists.  time_encoder.W is frozen
 * (requires_grad=False): its gradient and moments are ignored and may be NULL.  FFD_ERR_STATE: a call that needs a
 * tensor that is not bound.  ffd_train_create returns the object even on failure so that the message can be read
 * (ffd_train_last_error); FFD_ERR_HIP without a device, after the descriptor's own errors.
 * The workspace (activations kept for the backward, gradients of activations, wgrad partials) belongs to the object and
 * grows with B; its size is the query's.  The first batch call at a larger B than any before reallocates it, and the
 * first call after a bind rebuilds the tensor table: both synchronise with the device once (hipDeviceSynchronize,
 * hipFree, hipMalloc, one blocking copy).  Every other call only enqueues. */
typedef struct ffd_train ffd_train;
int ffd_train_create(ffd_train** out, const ffd_model_desc* desc, double dropout, int device);
void ffd_train_destroy(ffd_train* tr);
const char* ffd_train_last_error(const ffd_train* tr);
size_t ffd_train_work_bytes(const ffd_model_desc* desc, int B);
int ffd_train_bind(ffd_train* tr, const char* name, float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n);
/* The training forward (it keeps what the backward needs) at x (B, L, C) and the per-sample times: a second
 * implementation of ffd_score_forward_ts on the bound parameters, for tests. */
int ffd_train_forward(ffd_train* tr, const float* x, const float* timesteps, float* score_out, int B, void* stream);
/* A parameter-only binding, for inference use of the training forward and of ffd_train_input_vjp: no gradient and no
 * moments.  While any trainable tensor is bound this way, ffd_train_loss_grad, ffd_train_step, ffd_train_adamw and
 * ffd_train_grad_sqnorm answer FFD_ERR_STATE before any device work.  ffd_train_bind binds the tensor fully again. */
int ffd_train_bind_params(ffd_train* tr, const char* name, float* param, size_t n);
/* The vector-Jacobian product of the score with respect to its INPUT: dx_out = J^T v, J = d score / d x, v and dx_out
 * (B, L, C), through the activations that the object's last ffd_train_forward or ffd_train_loss_grad at this B left
 * in the workspace; FFD_ERR_STATE if there was none, if it failed, if B differs, or if ffd_train_adamw / ffd_train_step
 * has updated the parameters since (the activations are then no longer those of the weights the dgrads read).
 * It is the backward chain of ffd_train_loss_grad without any weight gradient, plus one more dense dgrad through
 * embedder.weight (the MLP: M = B, K = L C).  It reads parameters only: no gradient buffer, moment or parameter is
 * written.  v is not modified; dx_out must not be v.  Stream ordered, no host synchronisation. */
int ffd_train_input_vjp(ffd_train* tr, const float* v, float* dx_out, int B, void* stream);
/* Forward + backward for one batch: perturbation, training forward, per-sample losses (B doubles, as ffd_sm_eval_batch
 * with reduce_mean = 1) and the gradient of their mean into every bound gradient buffer (overwritten, not accumulated).
 * timesteps, mean_coeff, sigma: (B), in batch order.  index == NULL: x0 is (B, L, C) and sample b draws as global sample
 * sample_offset + b.  index (B) int64 on the device: x0 is the DATA SET and sample b is its row index[b], drawing as
 * global sample sample_offset + index[b] -- a row's noise does not depend on the batch it is in, and a shuffled batch
 * needs no gather (its times: ffd_sm_draw_times_at).  Every index must lie within the data set's rows (the caller's
 * contract, like a buffer's length: it is not checked on the device).  z (B, L, C) or NULL is in batch order. */
int ffd_train_loss_grad(ffd_train* tr, const float* x0, const int64_t* index, const float* timesteps,
                        const float* mean_coeff, const float* sigma, const float* z, uint64_t seed, uint64_t sample_offset,
                        int likelihood_weighting, double* per_sample_out, int B, void* stream);
/* The squared 2-norm of all bound gradients: one double on the device (two fixed-order fp64 trees). */
int ffd_train_grad_sqnorm(ffd_train* tr, double* sqnorm_out, void* stream);
/* AdamW on every bound trainable tensor in one launch (the arithmetic of ffd_adamw). */
int ffd_train_adamw(ffd_train* tr, const double* sqnorm, const ffd_adamw_cfg* cfg, void* stream);
/* A whole training step: the three calls above in order, the norm kept in the object.  The same bits as the calls made
 * separately. */
int ffd_train_step(ffd_train* tr, const float* x0, const int64_t* index, const float* timesteps, const float* mean_coeff,
                   const float* sigma, const float* z, uint64_t seed, uint64_t sample_offset, int likelihood_weighting,
                   double* per_sample_out, int B, const ffd_adamw_cfg* cfg, void* stream);

/* CRF capture inside ffd_sample_batch (the reference's cache.update_crf call, sampler.py:70-73):
 * on cached steps whose global step g satisfies g % every == 0 the (NL, L, d) CRF (score_models.py:181-194)
 * is written to ring slot (g / every) % n_slots; `last` receives the CRF of the last step of each
 * ffd_sample_batch call with g % last_every == 0 (E2CRFCache.crf_cache, caching.py:474-484).  Either pointer may
 * be NULL; cfg == NULL switches capture off.  Buffers are caller-owned device memory. */
typedef struct {
  float* ring;
  int32_t n_slots;
  int32_t every;
  float* last;
  int32_t last_every;
  int32_t reserved;
} ffd_crf_capture_cfg;
int ffd_cache_crf_capture(ffd_ctx* ctx, const ffd_crf_capture_cfg* cfg);

/* ---- the sampling loop -------------------------------------------------- */

/* E2CRFCache lifecycle used by DiffusionSampler (sampler.py:37-39,151-153):
 * enable/disable (score_models.py:202-289), reset (caching.py:115-129). */
int ffd_cache_enable(ffd_ctx* ctx, const ffd_cache_cfg* cfg);
int ffd_cache_disable(ffd_ctx* ctx);
int ffd_cache_reset(ffd_ctx* ctx);
/* K and R the gate of ffd_sample_batch uses from now on, WITHOUT touching tables or counters: the
 * reference evaluates determine_recompute_set on the sampler's current score_model.cache
 * (sampler.py:179-200), which a later enable_caching(**kwargs) replaces while the layers stay bound to
 * the first cache's tables (score_models.py:232). */
int ffd_cache_configure(ffd_ctx* ctx, const ffd_cache_cfg* cfg);
int ffd_cache_stats_get(const ffd_ctx* ctx, ffd_cache_stats* out);
/* Copy the (NL,H,L,hd) K and V tables (caching.py:88-91; zeros until step 0 ran) into
 * caller-owned device buffers; stream ordered.  Requires ffd_cache_enable. */
int ffd_cache_tables_read(ffd_ctx* ctx, float* k_out, float* v_out, void* stream);

/* THE RULES EVERY LOOP ENTRY SHARES (ffd_sample_batch and its _ode, _pc, _cond and _resample forms; each entry's own
 * comment states only what it adds).  An entry runs iterations [first, first + n_run) of its grid -- reverse steps,
 * the ODE's intervals, or resampling's visits -- on x (B,L,C) in place, enqueuing every kernel on `stream` with no host
 * synchronisation (one sync only when the timestep grid differs from the previous call's).  A run split into calls at
 * any iteration boundary gives the bits of one call.
 *   Arguments.  timesteps: host array (n_steps) = noise_scheduler.timesteps (sde.py:62-64); the caller supplies it
 *     because torch.linspace's last-ulp rounding depends on the host's vector width; step_size = timesteps[0] -
 *     timesteps[1] in fp32.  x must already hold the prior sample (ffd_prior) or the state after iteration first - 1.
 *   Draws.  z_inject == NULL: Philox on the device, keyed (seed, stream tag, global element index) as in ffd_sde_step;
 *     the predictor's tag is the iteration's index, the other updates' tags are their entries'.  Otherwise z_inject holds
 *     one (B,L,C) slab of N(0,1) draws per update, flat, in the order the call consumes them, starting at `first`.
 *   Cache gate.  use_cache 0/1 (requires ffd_cache_enable; the transformer only); global_step0 is the reference's
 *     global_step (sampler.py:130,210) at `first`.  An iteration's FIRST score evaluation follows
 *     ffd_host_gate at global step global_step0 + (iteration - first); every later evaluation of the iteration (Heun's
 *     second, the correctors' behind the first, the predictor's behind them) is a pure cache hit (n_recompute = 0).
 *     Tables and counters are those of ffd_score_forward_cached calls of these sizes in this order.
 *   CRF capture (ffd_cache_crf_capture).  Taken from the gated evaluation only, at its global step.
 *   FreSca (ffd_fresca_enable).  Applied to every evaluated score with h(t) of that evaluation's time.
 *   Errors.  FFD_ERR_INVALID -- null pointers, B < 1, a range outside the grid, step_size <= 0, what the entry adds --
 *     FFD_ERR_UNSUPPORTED (use_cache on another backbone) and FFD_ERR_STATE (use_cache without ffd_cache_enable) come
 *     back before any device work: nothing is launched and x stays as it is.
 *
 * ffd_sample_batch: one batch of DiffusionSampler.sample's inner loop (sampler.py:156-210), Euler-Maruyama steps
 * [first_step, first_step + n_run) of an n_steps-step reverse diffusion; one draw per step, z_inject (n_run,B,L,C). */
int ffd_sample_batch(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                     int first_step, int n_run, uint64_t seed, uint64_t sample_offset, const float* z_inject,
                     int use_cache, int global_step0, void* stream);

/* The same loop on the probability-flow ODE (see ffd_ode_step): an extension beyond the reference for sampling with
 * few score evaluations.  Deterministic: no noise, no seed.  The solvers walk the n_steps - 1 INTERVALS of the grid
 * t_0 = 1 ... t_{n_steps-1} = eps (interval i: from timesteps[i] to timesteps[i+1], width step_size) and end exactly
 * at eps; this call runs intervals [first_step, first_step + n_run), first_step + n_run <= n_steps - 1, n_steps >= 2.
 *   FFD_SOLVER_ODE_EULER  one score evaluation per interval (at timesteps[i]);
 *   FFD_SOLVER_ODE_HEUN   two: the predictor's at timesteps[i], the corrector's at (x_pred, timesteps[i+1]);
 *   FFD_SOLVER_ODE_AB2, FFD_SOLVER_DPMPP_2M  one (at timesteps[i]), reused by the next interval: the multistep solvers of
 *                         ffd_ode_multistep_step, with ffd_host_multistep_coef(timesteps[i-1], timesteps[i],
 *                         timesteps[i+1], step_size).  Cache gate, CRF capture and FreSca as for FFD_SOLVER_ODE_EULER.
 *                         The history q lives in the context.  first_step == 0 starts a trajectory without history;
 *                         first_step > 0 continues one, and is FFD_ERR_STATE (before any device work) unless the
 *                         context's previous sampling-loop call was ffd_sample_batch_ode with the same solver and B
 *                         and ended at interval first_step.  Every other loop entry (ffd_sample_batch, _pc, _cond, the
 *                         Euler / Heun solvers) drops the history.  A trajectory split into calls gives the bits of
 *                         one call.
 * Time-embedding table, stream ordering, cache gate, CRF capture and FreSca: the shared rules above (the global step
 * counts intervals; Heun's corrector evaluation is the pure hit).  With the unembedding fused into the tail (see
 * "fuse_tail") no score reaches HBM.
 * FFD_ERR_INVALID before any device work: the shared cases, and an unknown solver. */
enum { FFD_SOLVER_EULER_MARUYAMA = 0, FFD_SOLVER_ODE_EULER = 1, FFD_SOLVER_ODE_HEUN = 2 };
enum { FFD_SOLVER_ODE_AB2 = 4, FFD_SOLVER_DPMPP_2M = 5 }; /* (3 is FFD_SOLVER_PC) */
int ffd_sample_batch_ode(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                         int first_step, int n_run, int solver, int use_cache, int global_step0, void* stream);

/* The log-likelihood loop (see ffd_loglik_tail): the probability-flow ODE integrated the OTHER way, from eps up to 1,
 * with the divergence of its drift accumulated.  x (B,L,C) holds the series in the diffused domain at eps and is advanced
 * in place (after the grid's last interval it is the latent x_T); delta (B doubles, device) is ACCUMULATED, not zeroed,
 * so a trajectory can be split over calls at any interval boundary (the bits of one call).  log p(x) = ffd_prior_logp(x_T)
 * + delta.  The scheduler's descending fp32 grid timesteps[0..n_steps) is walked from its last point to its first:
 * interval j runs from timesteps[n_steps-1-j] to timesteps[n_steps-2-j]; its width is the difference of the two fp32
 * values formed in double (no scalar step_size: a non-uniform grid works).  This call runs intervals [first_interval,
 * first_interval + n_run), first_interval + n_run <= n_steps - 1, n_steps >= 2.
 *   solver        FFD_SOLVER_ODE_EULER (one divergence evaluation per interval) or FFD_SOLVER_ODE_HEUN (two, on the
 *                 augmented state (x, delta); v1 per sample in double) only;
 *   n_probes      k >= 1; every evaluation is ONE score evaluation at the stacked batch of (1 + 2 k) B rows, which must
 *                 pass the context's batch limits;  fd_rel: h = fd_rel sigma(t) per evaluation (ffd_host_loglik_h);
 *   probe_inject  NULL: fresh Rademacher draws per evaluation under (seed, sample_offset) and the tag plan above -- on a
 *                 fixed grid independent errors average out -- or one (n_probes, B, L, C) slab set per evaluation, flat, in
 *                 consumption order, starting at first_interval.
 * Every backbone.  No fused tail: the tail reads the stacked score from HBM (one pass over (rows, L, C) per evaluation,
 * far less than the forward it follows).  The perturbation and tail launches are timed under FFD_K_SDE; the tail that
 * ffd_kernel_work names is left as the last sampling loop set it.
 * FFD_ERR_INVALID before any device work: the shared cases (a null pointer, B < 1, a range outside the grid), n_probes
 * < 1, a solver outside the two, fd_rel <= 0 or non-finite, times of the run that are not finite, >= 0 and strictly
 * decreasing, a run whose largest e n_probes + m reaches 0x0FFFFFF0; FFD_ERR_UNSUPPORTED: (1 + 2 k) B L C >= 2^31 or a
 * stacked batch over the context's limit; FFD_ERR_STATE: FreSca on (a rescaled score is not the model's ODE; call
 * ffd_fresca_disable).  There is no cache argument, as for ffd_sample_batch_resample: the E2-CRF gate and tables assume
 * that time only falls, every evaluation here is the uncached forward, and the context's cache state -- enabled or not --
 * is left untouched. */
int ffd_loglik_batch(ffd_ctx* ctx, float* x, double* delta, int B, const float* timesteps, int n_steps, int first_interval,
                     int n_run, int solver, int n_probes, double fd_rel, const float* probe_inject, uint64_t seed,
                     uint64_t sample_offset, void* stream);

/* Predictor-corrector sampling (see ffd_langevin_step): ffd_sample_batch with n_corrector Langevin corrector steps in
 * front of every Euler-Maruyama step, in score_sde's order.  Reverse step i:
 *   1. n_corrector corrector steps at timesteps[i], each with its own score evaluation and its own draw (stream tag
 *      0x80000000 + i * n_corrector + j for corrector j);
 *   2. the unchanged Euler-Maruyama predictor at timesteps[i] on a fresh score evaluation (stream tag i: its noise is
 *      the noise of ffd_sample_batch).
 * n_corrector == 0 IS ffd_sample_batch (the call is forwarded).  Arguments as there, and
 *   snr, norm  the corrector's signal-to-noise ratio (> 0) and FFD_LANGEVIN_NORM_*;
 *   z_inject   NULL or (n_run, n_corrector + 1, B, L, C): per step the correctors' draws in order, then the predictor's.
 * Cache gate, CRF capture and FreSca: the shared rules above (the first corrector's evaluation is the gated one).
 * The corrector reads its score from HBM (three small launches behind the unembedding); the predictor keeps the fused
 * tail ("fuse_tail").
 * FFD_ERR_INVALID before any device work: as ffd_sample_batch, and n_corrector < 0, snr <= 0, an unknown norm,
 * n_steps * n_corrector > 0x7FFFFFF0. */
enum { FFD_SOLVER_PC = 3 };
int ffd_sample_batch_pc(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                        int first_step, int n_run, int n_corrector, float snr, int norm, uint64_t seed,
                        uint64_t sample_offset, const float* z_inject, int use_cache, int global_step0, void* stream);

/* Conditional sampling by replacement (see ffd_cond_project): ffd_sample_batch_pc with one projection onto the
 * observation after every state update.  Reverse step i is the predictor-corrector step as it stands; after each of
 * its n_corrector + 1 updates (corrector k = 0 .. n_corrector - 1, then the predictor, k = n_corrector) one
 * ffd_cond_project runs at timesteps[i] -- score_sde's order and time level -- with the context's SDE and G.
 *   cond       NULL: the call IS ffd_sample_batch_pc (forwarded; with n_corrector == 0 that is ffd_sample_batch).
 *              Otherwise obs / mask / std / obs_batch / domain as in ffd_cond_project, L and C the model's;
 *              final_replace != 0: when the call's last step is the grid's last step, one more projection with
 *              noiseless = 1 (the observed points come back exact to transform rounding).
 *   z_inject   NULL or (n_run, n_corrector + 1, 2, B, L, C): per update its own draw, then its projection's.
 * Stream tags: the predictor's i, the corrector's 0x80000000 + i * n_corrector + k, the projection's
 * 0xC0000000 + i * (n_corrector + 1) + k; n_steps * (n_corrector + 1) <= 0x3FFFFFF0 keeps the three ranges and the
 * reserved 0xFFFFFFFD .. 0xFFFFFFFF apart.  n_corrector == 0 is allowed (predictor + projection).
 * Cache gate, CRF capture, FreSca, the predictor's fused tail and ffd_async_status are those of ffd_sample_batch_pc; the
 * projection is one more launch behind the tail, timed under FFD_K_SDE.  The ODE solvers have no conditional form
 * (score_sde defines replacement for predictor-corrector samplers only).
 * FFD_ERR_INVALID before any device work: as ffd_sample_batch_pc and ffd_cond_project, and n_steps * (n_corrector + 1)
 * > 0x3FFFFFF0; FFD_ERR_UNSUPPORTED: a frequency-domain length outside its set. */
typedef struct {
  const float* obs;
  const float* mask;
  const float* std;
  int32_t obs_batch;
  int32_t domain;        /* FFD_COND_* */
  int32_t final_replace;
  int32_t reserved;
} ffd_cond_cfg;
int ffd_sample_batch_cond(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                          int first_step, int n_run, int n_corrector, float snr, int norm, uint64_t seed,
                          uint64_t sample_offset, const float* z_inject, int use_cache, int global_step0,
                          const ffd_cond_cfg* cond, void* stream);

/* Resampled conditional sampling ("time travel": RePaint, Lugmayr et al. 2022; an extension).  Replacement draws the
 * observed part of the state independently of the unobserved part, which on a forecast leaves an error that more steps
 * do not remove.  Here the grid's N = n_steps reverse steps are cut into blocks [0, j), [j, 2j), ... (j = jump; the last
 * block may be shorter, jump > N is one block) and every block is run r = resample times: between two passes of the
 * block [i0, e) the whole state is diffused forward again, by one ffd_forward_transition from s = timesteps[e] (0 when
 * e == N) to t = timesteps[i0].  No projection follows the transition: its observed part is a valid noised observation.
 * The schedule has U = r N visits and (r - 1) ceil(N / j) transitions; a transition belongs to the visit it follows.
 * ffd_host_resample_visits returns U.  ffd_host_resample_visit: *step_out = the grid index visit `visit` runs,
 * *back_to_out = -1 or the grid index i0 the state is re-noised to after it.  Host only; FFD_ERR_INVALID: n_steps, jump,
 * resample < 1, U > INT_MAX, a visit outside [0, U), a null pointer.
 * ffd_sample_batch_resample walks visits [first_visit, first_visit + n_visits).  A visit IS reverse step
 * timesteps[step] of ffd_sample_batch_cond -- correctors, predictor with its fused tail, one projection behind every
 * update -- with the visit ordinal u in place of the step index in the three stream tags; transition q (counted in
 * schedule order from 0) draws under tag 0xE0000000 + q, and U (n_corrector + 1) <= 0x1FFFFFF0 keeps the projections'
 * tags below it.  The transition is timed under FFD_K_SDE.
 *   z_inject   NULL or flat in execution order: per visit (n_corrector + 1, 2, B, L, C) as for ffd_sample_batch_cond,
 *              then one more (B, L, C) slab if a transition follows the visit; the pointer starts at first_visit.
 *   cond       required (FFD_ERR_INVALID when NULL); final_replace runs after visit U - 1 only.
 * resample == 1 is ffd_sample_batch_cond(use_cache = 0) bit for bit, and a run split over calls at any visit boundary
 * is bit-identical to the unsplit run.  There is no cache argument: the E2-CRF gate and tables assume that time only
 * falls; the context's cache state is left untouched.  The ODE solvers have no resampled form.
 * FFD_ERR_INVALID before any device work: as ffd_sample_batch_cond, and jump, resample < 1, a visit range outside
 * [0, U], U (n_corrector + 1) > 0x1FFFFFF0, and -- checked for resample > 1 only, where transitions run -- timesteps
 * that are not finite, not non-increasing (equal neighbours are accepted) or below 0. */
int ffd_host_resample_visits(int n_steps, int jump, int resample);
int ffd_host_resample_visit(int n_steps, int jump, int resample, int visit, int* step_out, int* back_to_out);
int ffd_sample_batch_resample(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                              int first_visit, int n_visits, int jump, int resample, int n_corrector, float snr, int norm,
                              uint64_t seed, uint64_t sample_offset, const float* z_inject, const ffd_cond_cfg* cond,
                              void* stream);

/* Guided conditional sampling (see ffd_guide_seed): Euler-Maruyama steps whose score is steered by the gradient of
 * the reconstruction loss through the score model.  Reverse step i at t = timesteps[i]:
 *   1. s = score(x, t);  2. ffd_guide_seed -> u, v, the loss;  3. jtv = J^T v (the score model's input VJP);
 *   4. ffd_guide_combine with ffd_host_guide_coef(t)'s alpha and lambda -> s~;  5. the stand-alone ffd_sde_step with s~
 *   (stream tag i);  6. guide->replace != 0: one ffd_cond_project at t (stream tag 0xC0000000 + i).
 * The tags are those of ffd_sample_batch_cond with n_corrector = 0.  When the call's last step is the grid's last step
 * and cond->final_replace != 0, one noiseless projection ends the run.
 *   ctx        the SDE and G; for FFD_MODEL_MIXTURE also the score and its VJP (net is ignored)
 *   net        the transformer and the MLP: an ffd_train bound to the context's parameters (ffd_train_bind_params is
 *              enough) supplies the forward and the VJP -- FFD_ERR_STATE when NULL, FFD_ERR_INVALID when its descriptor
 *              differs from the context's.  The LSTM has no backward: FFD_ERR_UNSUPPORTED.
 *   cond       required: obs / mask / std / obs_batch / domain / final_replace as in ffd_sample_batch_cond
 *   guide      required: scale, obs_var, rho >= 0 of lambda(t); obs_var is in the units of the diffused domain
 *   z_inject   NULL or (n_run, 1, 2, B, L, C): per step the predictor's draw, then the projection's slab (read only with
 *              replace)
 *   loss_out   NULL or (n_run, B) doubles on the device: the loss BEFORE each step of the call
 * The shared loop rules hold: no host synchronisation, and a run split over calls at any step boundary gives the bits
 * of one call.  scale = 0 with replace is ffd_sample_batch_cond(n_corrector = 0, use_cache = 0) bit for bit on the
 * mixture.  No cache argument (the context's cache state is left untouched), no correctors, ODE solvers or resampling;
 * FFD_ERR_STATE before any device work while FreSca is on.
 * FFD_ERR_INVALID before any device work: the shared cases, a NULL cond or guide, ffd_cond_project's cases, a
 * non-finite or negative scale, obs_var or rho, a step of the run whose lambda has a zero denominator, n_steps >
 * 0x3FFFFFF0, x aliasing z_inject. */
typedef struct {
  double scale, obs_var, rho;
  int32_t replace;
  int32_t reserved;
} ffd_guide_cfg;
int ffd_sample_batch_guided(ffd_ctx* ctx, ffd_train* net, float* x, int B, const float* timesteps, int n_steps,
                            float step_size, int first_step, int n_run, uint64_t seed, uint64_t sample_offset,
                            const float* z_inject, const ffd_cond_cfg* cond, const ffd_guide_cfg* guide, double* loss_out,
                            void* stream);

/* ---- class-conditional score models and classifier-free guidance (Ho & Salimans 2022; an extension) ----
 * A learned table class_embedding.weight (n_classes + 1, d_model) whose row n_classes is the NULL class (unconditional).
 * Sample b with label y_b evaluates the network with table[y_b] added to its time embedding, i.e. every token is
 * h = embed(x) + pos + temb(t_b) + table[y_b].  Labels are int32; -1 and n_classes both mean null.  The guided score is
 * diffusers' convention  s~ = s_u + g (s_c - s_u):  g = 1 the conditional score and g = 0 the unconditional one, one
 * evaluation of B rows each; any other g one evaluation at the stacked batch of 2 B rows (conditional block first).
 *
 * The four operators need no context (ffd_class.hip):
 *   ffd_class_temb        out[r, :] = temb[r * temb_stride + :] + table[label_r, :] for r < B (temb_stride 0: one shared
 *                         row, or d); stack = 1: rows B .. 2B - 1 get temb[r - B] + table[null].  labels NULL: every row
 *                         null.  out may be temb when temb_stride == d and stack == 0.  A label outside [-1, n_classes]
 *                         reads the null row (the entry points that take labels from a caller refuse it beforehand).
 *   ffd_cfg_combine       c[i] = fmaf(g, c[i] - u[i], u[i]) over n floats, in place on c (the subtraction rounded on its
 *                         own); c and u need 4-byte alignment only and must not overlap.  An element's bits do not
 *                         depend on n or on the alignment.
 *   ffd_class_drop        the training-time label dropout: out[b] = n_classes where the U[0, 1) draw of global row
 *                         sample_offset + row_b under (seed, stream tag 0xFFFFFFFC) is < p_uncond, else labels[row_b] (a
 *                         null label stays n_classes or -1 as given); row_b = index[b], or b when index is NULL: the
 *                         row keying of ffd_sm_draw_times_at (slot g & 3 of Philox block g >> 2, u = (w >> 8) 2^-24).
 *                         labels NULL: out[b] = n_classes.  0 <= p_uncond <= 1 (1: every row dropped).
 *   ffd_class_table_grad  dtable[c, j] = sum over {b : eff_label_b == c} of dtemb[b, j], b in order, accumulated in fp64,
 *                         no atomics; labels -1 count as n_classes; all n_classes + 1 rows are written (absent: 0).
 * FFD_ERR_INVALID: a null pointer (labels / index where optional excepted), B, d or n_classes < 1, temb_stride not 0 or
 * d, an in-place ffd_class_temb that is not the allowed one, a non-finite g, n == 0, p_uncond outside [0, 1].
 *
 * Context state: ffd_class_enable / ffd_class_disable, the same kind of state as FreSca.  The table pointer is read
 * live at every evaluation and never copied (a training update is seen); labels_host is the host copy of `labels`
 * that ffd_class_enable validates -- it is not kept.  labels == NULL: every sample null (n_labels and labels_host are
 * then ignored).  While the state is on:
 *   - all three network kinds honour it in ffd_sample_batch, _ode (every solver), _pc, _cond and _resample: each
 *     evaluation builds the (B or 2 B, d) embedding table from the time-table row, evaluates B or 2 B rows, combines
 *     -- on the final hidden rows where the tail is fused, else on the score: the unembedding is affine and the two
 *     weights sum to 1, so that is exact in real arithmetic -- and hands B rows to the unchanged tail and FreSca.  The
 *     batch limit and the workspace are those of 2 B rows when g is neither 0 nor 1.  These loops run single-stream
 *     (no CU partitions).
 *   - ffd_score_forward_ts and ffd_sm_eval_batch evaluate the conditional branch only (guidance_scale is ignored).
 * FFD_ERR_INVALID (ffd_class_enable): a NULL cfg or table, n_classes < 1, labels without labels_host, n_labels < 1, a
 * label outside [-1, n_classes], a non-finite guidance_scale; FFD_ERR_UNSUPPORTED: the mixture kind.
 * Refused before any device work while the state is on: FFD_ERR_INVALID n_labels != B (loops, ffd_score_forward_ts,
 * ffd_sm_eval_batch); FFD_ERR_STATE use_cache (or a cached n_recompute), ffd_score_forward, ffd_score_forward_cached,
 * ffd_loglik_batch, ffd_sample_batch_guided. */
typedef struct {
  const float* table;         /* device (n_classes + 1, d_model) */
  const int32_t* labels;      /* device (n_labels) or NULL */
  const int32_t* labels_host; /* host copy of labels (validated, not kept) */
  int32_t n_classes;
  int32_t n_labels;
  float guidance_scale;
  int32_t reserved;
} ffd_class_cfg;
int ffd_class_enable(ffd_ctx* ctx, const ffd_class_cfg* cfg);
int ffd_class_disable(ffd_ctx* ctx);
int ffd_class_temb(const float* temb, int temb_stride, const float* table, int n_classes, const int32_t* labels, int B, int d,
                   int stack, float* out, void* stream);
int ffd_cfg_combine(float* c, const float* u, float g, size_t n, void* stream);
int ffd_class_drop(const int32_t* labels, int n_classes, const int64_t* index, int B, double p_uncond, uint64_t seed,
                   uint64_t sample_offset, int32_t* out, void* stream);
int ffd_class_table_grad(const float* dtemb, const int32_t* eff_labels, int n_classes, int B, int d, float* dtable,
                         void* stream);

/* Training with classes.  ffd_train_classes (before the first bind; FFD_ERR_STATE after one, FFD_ERR_INVALID n_classes <
 * 1 or a second call) appends class_embedding.weight (n_classes + 1, d_model) to the object's tensors: the gradient
 * norm, the clip and AdamW cover it like any other tensor, decay included.  ffd_train_labels sets the device labels of
 * the batches that follow, indexed like x0 (by `index` where one is given, else by the batch row), and the dropout
 * probability; labels NULL: every sample null.  n: the labels' length (rows of the data set or of the batch; the
 * caller's to keep within).  ffd_train_loss_grad and ffd_train_step use ffd_class_drop's labels (seed and
 * sample_offset of the call), ffd_train_forward the labels as they are.  The forward adds table[eff_label_b] to the
 * time encoder's dense output; the backward runs ffd_class_table_grad on the time embedding's gradient.  The
 * effective labels live outside the workspace: ffd_train_work_bytes does not change.  FFD_ERR_INVALID: n < 1 with
 * labels, p_uncond outside [0, 1]; FFD_ERR_STATE: ffd_train_labels without ffd_train_classes. */
int ffd_train_classes(ffd_train* tr, int n_classes);
int ffd_train_labels(ffd_train* tr, const int32_t* labels, size_t n, double p_uncond);

/* How the context's last sampling-loop call ran: *parts_out = 2 as two CU partitions (ffd_tune "partitions"), 1 on the
 * caller's stream alone. */
int ffd_partition_status(const ffd_ctx* ctx, int* parts_out);

/* What a sampling-loop call of B samples WOULD do under the calling thread's knobs, by the decision and the layer
 * planner the loops themselves run; nothing is launched (the first call on a context creates the two CU-masked streams
 * and their events, as the first eligible loop call would).  entry: FFD_SOLVER_EULER_MARUYAMA = ffd_sample_batch with
 * device draws, FFD_SOLVER_ODE_EULER = ffd_sample_batch_ode's Euler solver; every other FFD_SOLVER_* value names a loop
 * that never partitions (parts = 1, halves not planned).  The call's own state -- z_inject, use_cache, a capturing
 * stream -- is not part of the question: such a call stays single-stream whatever this reports.
 *   parts            2: as two CU partitions | 1: on the caller's stream (ffd_partition_status's encoding);
 *   cu_budget        CUs per half (128 on MI355X); 0 where no partitions exist (the device's CUs do not halve, or the
 *                    question never got that far: "partitions" = 0, B < 2, another backbone, cache / FreSca / timing on);
 *   half[0], half[1] samples [0, ceil(B/2)) and the rest, planned for cu_budget CUs (halves_planned = 1; else only nb is
 *                    set).  They are planned -- and reported -- also where the decision is 1 because of them;
 *   whole            the single-stream plan of all B samples for the device's CUs (whole_planned = 1: a finalized transformer).
 * Per plan: nb samples; ffn / attn: the form names ffd_kernel_work gives ("k_qkv_attention" without its static-bound
 * suffix); nw waves per workgroup and cps chunks per ring slot (k_ffn_rows forms, else 0); mb 16-row tiles per workgroup
 * (k_ffn_ln forms, else 0) and the persist factor (k_ffn_ln behind k_linear_res_ln); hpw heads per attention workgroup,
 * qg q-tiles per wave, kspl key pieces of the small-batch split attention (0: one workgroup per head or head pair);
 * part_floats: partial rows the form keeps in the shared workspace (non-zero: never partitioned); ffn_tiles / ffn_grid:
 * row tiles and workgroups of the FFD_K_FFN launch as its launcher computes them (k_ffn_rows and k_ffn_ln forms; 0 for
 * the others), one_per_tile = 1 where they are equal, else the grid is the persistent one sized from the CU count.
 * FFD_ERR_INVALID: ctx or info NULL, B < 1, entry outside the FFD_SOLVER_* values. */
typedef struct ffd_partition_half {
  int nb;
  int nw, cps, mb, persist;
  int hpw, qg, kspl;
  int ffn_tiles, ffn_grid, one_per_tile;
  long long part_floats;
  char ffn[64], attn[48];
} ffd_partition_half;
typedef struct ffd_partition_info {
  int parts, cu_budget, halves_planned, whole_planned;
  ffd_partition_half half[2], whole;
} ffd_partition_info;
int ffd_partition_plan(ffd_ctx* ctx, int B, int entry, ffd_partition_info* info);

/* Tuning knobs for experiments and for the test suite's kernel variants (results stay within the parity tolerance,
 * only the kernel choice / tiling changes).  PER CALLING THREAD since round 4 (thread_local): a knob set on one thread
 * selects kernels for the launches THAT thread makes and is invisible to every other thread, so two samplers on two
 * threads cannot disturb each other; a thread starts from the defaults.  ffd_tune_get reads the calling thread's value.
 *   "ffn_mb" = 0 (heuristic) | 1 | 2 | 3 | 4   rows/16 per workgroup of k_ffn_ln;
 *   "ffn_height" = 1 | 2 | 0                   where the 16-row tiles are 0.55 - 1 or 1.25 - 3 per CU (ECG: B = 12 ... 21 and
 *                                              28 ... 65, the reference's default sample_batch_size of 50 among them):
 *                                              k_ffn_ln at 16 / 32 / 48 rows per workgroup, one tile per CU, with the
 *                                              out-projection + LN1 inside (1) or behind a k_linear_res_ln launch (2) |
 *                                              0: the small-batch pair / sliced forms;
 *   "reset" (value ignored)                    every knob below back to its default;
 *   "ffn_rows" = 1 | 0 | 2                     FFN at large M (d_model 72 / 64 / 60 / 48): row-owning waves + CU-shared LDS weight ring
 *                                              (k_ffn_rows, ffd_ffn_rows.hip) or the F-split workgroup (k_ffn_ln); 2 = at
 *                                              every M where the small- / mid-batch forms are off (test suite);
 *   "rows_slices_fuse" = 0 (by estimate) | 1 | 2 sliced form of k_ffn_rows: the out-projection + LN1 inside every unit (1) or as
 *                                              one k_linear_res_ln launch in front of slices without that slot (2);
 *   "ffn_rows_nw" = 0 (heuristic) | 4 | 8 | 12 waves per workgroup of k_ffn_rows (a tile is 32 rows per wave);
 *   "ffn_rows_cps" = 0 | 2 | 1                 32-unit chunks per ring slot (= per barrier) of k_ffn_rows (default 2);
 *   "ffn_rows_fuse" = 1 | 0                    out-projection + residual + LN1 inside k_ffn_rows (one more ring slot per
 *                                              tile; two-chunk slots only) or k_linear_res_ln in front of it;
 *   "rows_slices" = 0 (heuristic) | -1 | 2..32 mid-size M: the fused kernel over tiles x slices of the hidden dimension
 *                                              (one unit per CU) + a reduce / LN2 launch; -1 = never, n = n slices forced;
 *   "ffn_persist" = 1 | 0 | n                  k_ffn_ln at large M: persistent grid (n x resident workgroups) or one workgroup per tile;
 *   "small_path" = 1 | 0                       small M: out-proj + LN1 + FFN + LN2 with F split over up to 16 workgroups per
 *                                              16-row tile and a reduce + LN2 launch (ffd_small.hip); "small_wgs" = n: most
 *                                              workgroups the split form is used for (0 = heuristic);
 *   "mid_path" = 1 | 0 | 2 | 4 | 8            mid-size M: the 64-row FFN main loop over F slices + the reduce launch
 *                                              (1 = where the round model says it pays, n = force n slices);
 *   "ffn_split" = 0 | 1                        OPT-IN, off by default: the FFN on the bf16 matrix cores, every fp32 operand cut
 *                                              into three bf16 parts and the six largest cross terms kept (fp32-equivalent to
 *                                              ~2e-7, passes the same goldens; NOT the reference's fp32 FMA arithmetic);
 *                                              needs d_model <= 96, dim_feedforward % 128 == 0 (ffd_ffn_split.hip);
 *   "embed_threads" = n                        threads the embedding kernel's grid aims at (default 262144); "embed_ldsx" = 1 | 0:
 *                                              a wave's shared x rows through LDS or per-lane loads;
 *   "attn_small" = 1 | 0 | 2 | 4               small batches: several workgroups per (sample, head), the key range of a
 *                                              q-tile cut into 2 / 4 pieces over the waves (1 = by batch size, 0 = never);
 *   "ffn_rem" = 1 | 0                          d%16 remainder rows of GEMM2 on the 4x4x1 MFMA;
 *   "lstm_wave" = 1 | 0                        LSTM: all layers as a wavefront of (16-sample tile, layer) workgroups
 *                                              (k_lstm_wave, every batch), or the per-layer kernels (0: the test
 *                                              suite's cross-check; 2 is accepted and means 1);
 *   "lstm_wave_fault" = n, "lstm_wave_spin_ms" = ms   tests: unit n - 1 of k_lstm_wave withholds its progress word / the
 *                                              time limit of one wait on such a word (see ffd_async_status);
 *   "fail_alloc_after" = n                     tests: the n-th device allocation from now fails with FFD_ERR_NOMEM;
 *   "lstm_wave_persist" = 1 | 0                one launch whose resident workgroups run (chunk, layer, tile) units in
 *                                              index order, or one launch per group of `per` layers;
 *                                              "lstm_wave_per" = n: at most n layers in flight (0 = as many as the CUs
 *                                              hold; tests); "lstm_wave_chunk" = 0 | 1 | even n: cell steps per
 *                                              unit where the (tile, layer) pairs outnumber the CUs (0: chosen so that
 *                                              the rounds come out whole, 1: layers walked whole, n: forced);
 *   "fuse_tail" = 1 | 0                        unembedding inside the SDE-step kernel of ffd_sample_batch (and of the
 *                                              predictor of ffd_sample_batch_pc) and the ODE tails of
 *                                              ffd_sample_batch_ode, the multistep ones included (no FreSca);
 *   "attn_fused" = 1 | 0                       in-projection + attention in one kernel (k_qkv_attention*);
 *   "attn_kvq" = 1 | 0                         small-batch split attention: tile 0 = k | v, tile 1 = q, q projected for a
 *                                              workgroup's own q-tiles only (head_dim 6 / 8) | the whole head;
 *   "attn_hpw" = 0 (heuristic) | 1 | 2         heads per workgroup of that kernel;
 *   "attn_qg" = 0 (heuristic) | 1 | 2 | 3      query tiles per wave;
 *   "partitions" = 1 | 0 | 2                   ffd_sample_batch (device draws) and ffd_sample_batch_ode (FFD_SOLVER_ODE_EULER) on a
 *                                              transformer without cache / FreSca / armed kernel timing: samples [0, ceil(B/2))
 *                                              and the rest as two chains on streams confined to disjoint halves of every
 *                                              XCD's CUs, forked from and joined to the caller's stream by events (same
 *                                              results bit for bit; every other case runs on the caller's stream).  1: where
 *                                              both halves take the row-owning FFN and fill their CUs; 2: wherever both
 *                                              halves take it; 0: never.  ffd_partition_status tells which path ran;
 *   "attn_static_bound" = 1 | 0                layers whose score bound holds from the weights alone (see
 *                                              ffd_host_attn_score_bound) run the fused kernels' instances without the
 *                                              per-launch bound (same results bit for bit) | every layer measures it;
 */
int ffd_tune(const char* key, int value);
int ffd_tune_get(const char* key, int* value);

/* ---- introspection for benchmarks --------------------------------------- */

/* Algorithmic FLOPs of one score evaluation per sample (SURVEY 8(d) formula) and of
 * the fused FFN kernel per launch at batch B. */
double ffd_flops_per_sample_step(const ffd_ctx* ctx, int cache_hit);
double ffd_ffn_flops_per_launch(const ffd_ctx* ctx, int B);
/* Kernel classes of the sampling path, for in-situ timing and roofline accounting. */
enum {
  FFD_K_FFN = 0,         /* k_ffn_ln: linear1 + relu + linear2 + residual + LayerNorm2 */
  FFD_K_ATTN = 1,        /* k_qkv_attention*: in-projection + attention (or the two-kernel fallback) */
  FFD_K_OUTPROJ = 2,     /* k_linear_res_ln: out-projection + residual + LayerNorm1 */
  FFD_K_LSTM_REC = 3,    /* k_lstm_*: the L-step recurrence of one residual LSTM layer */
  FFD_K_LSTM_GATES = 4,  /* k_linear_rm: input-gate GEMM of one LSTM layer */
  FFD_K_SDE = 5,         /* the SDE step (or the fused unembed + SDE step); in ffd_sample_batch_ode the ODE tails (Euler,
                          * Heun's two, or the multistep tail), in ffd_sample_batch_pc also the corrector's launches */
  FFD_K_EMBED = 6,
  FFD_K_UNEMBED = 7,
  FFD_K_COUNT = 8
};
/* Diagnostics of the LSTM layer wavefront (k_lstm_wave): with host_out == NULL, arm a trace of `capacity_units` units --
 * the k_lstm_wave launches of the next forward passes (first sub-batch each) then write four 64-bit words per work unit
 * (chunk, layer, tile), unit index = chunk * layers * tiles + layer * tiles + tile: 100 MHz real-time ticks at the unit's
 * start, after its start-up (weights, state, first rows in), at its end, and [47:0] ticks spent waiting on progress words
 * | workgroup << 48.  With host_out != NULL: synchronise, copy the records out (n_units_out = how many), disarm.  The
 * capacity must cover chunks * layers * ceil(B / 16) units of the traced launch. */
int ffd_lstm_trace(ffd_ctx* ctx, unsigned long long* host_out, int capacity_units, int* n_units_out);

/* In-situ timing: between _begin and _end every launch of a kernel whose class bit is set in
 * `class_mask`, issued by forward / sample calls on this context, is bracketed by a HIP event pair
 * on the launch stream (up to max_launches pairs in total); _end synchronises; _get returns the mean
 * duration and launch count of one class.  For bench.py's roofline lines. */
int ffd_kernel_timing_begin(ffd_ctx* ctx, uint32_t class_mask, int max_launches);
int ffd_kernel_timing_end(ffd_ctx* ctx);
int ffd_kernel_timing_get(const ffd_ctx* ctx, int kernel_class, float* avg_ms_out, int* launches_out);
/* Algorithmic work of ONE launch of a kernel class at batch B (SURVEY 8(d) figures: FLOPs for the
 * MFMA-bound classes, HBM bytes for all); cache_hit = 1 for a pure-cache step.  Returns the name of the
 * kernel(s) the forward pass plans for that class under the calling thread's ffd_tune knobs (static
 * string), or NULL for a class the forward does not launch at this batch.  FFD_K_SDE names the tail of the loop entry
 * the context ran last (Euler-Maruyama before any); for Heun, whose two tails differ, the mean of its two launches; for the
 * multistep solvers the tail with history (every interval of a trajectory but its first, which reads no history); after
 * ffd_sample_batch_pc the predictor's tail (its work figures) followed by the corrector's kernels.  The projections of
 * ffd_sample_batch_cond (k_cond_project / k_cond_time: about 16 B of HBM traffic per element, 12 B with device draws) and
 * the transitions of ffd_sample_batch_resample (the step kernel's OpTransition: 12 B per element, 8 B with device draws)
 * are timed under FFD_K_SDE as well but are NOT in this class's name or figures, which describe the update launches only:
 * after a conditional loop the mean of ffd_kernel_timing_get covers more launches than the figures do. */
const char* ffd_kernel_work(const ffd_ctx* ctx, int kernel_class, int B, int cache_hit, double* flops_out,
                            double* bytes_out);
/* Time `iters` runs of layer 0's FFN at batch B as the forward pass plans it (the launches
 * ffd_kernel_timing counts as FFD_K_FFN, named by ffd_kernel_work) on random rows, on `stream`
 * with HIP events; returns average milliseconds per run in *ms_out.  Synchronous (benchmark
 * helper only). */
int ffd_bench_ffn(ffd_ctx* ctx, int B, int iters, float* ms_out, void* stream);

/* Diagnostic: the shader clock the chip holds under the dominant kernel, and a timeline of one launch.  Launches layer
 * 0's FFN as the forward pass plans it at batch B back to back for `warm_seconds` on random data, then once more with
 * in-kernel stamps (s_memtime /
 * s_memrealtime, written to a scratch buffer nothing else reads); *ghz_out = median over workgroups of shader cycles
 * per 10 ns tick x 0.1 inside the main loop, *loop_us_out (may be NULL) = median time a workgroup spent in its main
 * loops.  raw_out (may be NULL): up to raw_capacity records of 8 x u64 per workgroup -- [0] main-loop shader cycles,
 * [1] main-loop 10 ns ticks, then chip-wide 100 MHz timestamps [2] entry, [3] / [4] first main loop begin / end,
 * [5] first epilogue end, [6] exit, and [7] tiles processed; *nwg_out = workgroups that ran.  FFD_ERR_UNSUPPORTED
 * (naming the form) where the planned form has no stamped twin (k_ffn_ln, k_ffn_rows and the split FFN have one).
 * Synchronous. */
int ffd_probe_ffn_clock(ffd_ctx* ctx, int B, double warm_seconds, double* ghz_out, double* loop_us_out,
                        unsigned long long* raw_out, int raw_capacity, int* nwg_out, void* stream);

/* Status of the stream-ordered work this context has enqueued, for the one failure a kernel can only report after
 * the fact: the LSTM backbone (LSTMScoreModule.forward, score_models.py:486-511) runs its layers as a wavefront of
 * workgroups that wait on each other's progress words inside ONE launch (k_lstm_wave).  That protocol needs the
 * launch's workgroups co-resident, i.e. THE DEVICE'S COMPUTE UNITS TO ITSELF: with another stream or process holding
 * compute units a wait can outlast its time limit (2 s per wait; ffd_tune "lstm_wave_spin_ms").  Such a wait is an
 * error, never a silent fall-through: the kernel records it, the launch drains, and the results of that launch are
 * invalid.  Returns FFD_ERR_STATE (message via ffd_last_error) once for such a launch, FFD_OK otherwise; call it after
 * synchronising the stream.  Every compute entry point makes the same check on entry, so the error also surfaces at
 * the next call.  (The reference has no counterpart: its nn.LSTM layers are separate stream-ordered kernels.) */
int ffd_async_status(ffd_ctx* ctx);

/* Diagnostic + benchmark helper for layer 0's attention launch as the forward pass plans it at batch B (the fused
 * in-projection + attention of ffd_qkvattn.hip where it exists, else the two-kernel form) on random rows (replaces nothing in the reference: measurement scaffolding for cached_transformer.py:228-311's
 * kernel).  n_recompute < 0: plain layer; otherwise the E2-CRF mode of that recompute-set size (needs ffd_cache_enable
 * and one FULL step for the tables).  Launches it back to back for `warm_seconds`, times `iters` launches with HIP
 * events (*ms_out = milliseconds per launch), then -- when raw_out != NULL -- once more as its stamped twin (d_model 72,
 * head_dim 6, one workgroup per head or head pair, q | k | v pack; FFD_ERR_UNSUPPORTED naming the form otherwise): up to raw_capacity records of 16 x u64 per WAVE: [0] 100 MHz real time at entry, shader-clock
 * (s_memtime) stamps [1] entry, [2] projection begin, [3] projection end, [4] attention begin, [5] attention end,
 * [6] exit, shader cycles summed over the wave's key tiles [7] K fragments + QK^T, [8] mask + softmax, [9] P.V,
 * [10] key tiles walked, [11] HW_ID, [12] 100 MHz real time at exit; *nrec_out = records written.  Synchronous. */
int ffd_probe_attn(ffd_ctx* ctx, int B, int n_recompute, double warm_seconds, int iters, float* ms_out,
                   unsigned long long* raw_out, int raw_capacity, int* nrec_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FFD_H */
