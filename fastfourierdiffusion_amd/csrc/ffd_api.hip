// libffd C ABI (include/ffd.h): context, weights, forward orchestration, E2-CRF cache
// state machine and the sampling loop.  Host code only launches kernels; there is no
// CPU compute path -- every entry point that needs the device fails loudly without one.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ffd.h"
#include "ffd_internal.h"

using namespace ffd;

namespace {

// A workspace buffer on the device that only grows (ensure); cap = the elements that p holds, 0 while there are none
template <typename T>
struct Grow {
  T* p = nullptr;
  size_t cap = 0;
};

// One parameter of the state dict: its key and size, the device copy ffd_load_weight made, and the field of
// ModelWeights / LayerWeights / LstmLayer / MlpLayer the launch sites read it from
struct WeightSlot {
  std::string key;
  size_t n;
  const float** field;
  float* dev = nullptr;
};

struct ModelWeights {
  const float *embed_w, *embed_b, *unembed_w, *unembed_b;
  const float* pos;  // transformer: positional table, renormalised in place by ffd_finalize_weights
  const float *time_W, *time_dense_w, *time_dense_b;
};

// torchvision.ops.MLP(d, [d_mlp, d]) = Sequential(Linear, ReLU, Dropout, Linear, Dropout): indices 0 and 3
struct MlpLayer {
  const float *w0, *b0, *w3, *b3;
};

// The Gaussian mixture behind FFD_MODEL_MIXTURE: means (K, L, C), log-weights (K), the shared variance (L, C)
struct MixtureWeights {
  const float *means, *logw, *var;
};

struct LstmLayer {
  const float *wih, *whh, *bih, *bhh;
  float *wih_p = nullptr, *bsum = nullptr;
  float *ih_wpk = nullptr, *hh_wpk = nullptr, *b_wpk = nullptr;  // k_lstm_wave's fragment-ordered packs (d_model % 4 == 0, >= 16)
};

__global__ void k_add_vec(const float* a, const float* b, float* o, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] + b[i];
}

__global__ void k_fill_hash(float* p, size_t n, uint32_t seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)i * 2654435761u ^ seed;
    h ^= h >> 16, h *= 0x85ebca6bu, h ^= h >> 13, h *= 0xc2b2ae35u, h ^= h >> 16;
    p[i] = ((float)(h >> 8) * (1.0f / 8388608.0f)) - 1.0f;  // uniform [-1, 1)
  }
}

}  // namespace

struct ffd_ctx {
  ffd_model_desc desc{};
  int device = 0;
  std::string err;
  std::vector<WeightSlot> weights;  // every parameter the model takes, bound once by ffd_create (bind_weights)
  std::vector<void*> owned;  // packed / table / workspace allocations
  bool finalized = false;
  ModelWeights model{};
  std::vector<LayerWeights> layers;  // one of the three, by desc.kind (sized by ffd_create: `weights` points into them)
  std::vector<LstmLayer> lstm;
  std::vector<MlpLayer> mlp;
  MixtureWeights mix{};    // FFD_MODEL_MIXTURE (no layers: the score is closed-form)
  Grow<float> mix_work;    // the mixture kernel's per-slice partials
  float* G_dev = nullptr;
  std::vector<float> G_host;
  // workspace (ensure_workspace; qkv, ffn_part and the LSTM wavefront's on first use)
  Grow<float> h0, h1, attn, score;
  Grow<float> qkv;      // head-major q / k / v of the two-kernel attention | LSTM gate pre-activations | MLP hidden (B, d_mlp)
  Grow<float> temb_b;   // (B, d) per-sample time embeddings (ffd_score_forward_ts)
  Grow<float> temb_tab, ts_dev;  // the trajectory's time embeddings (n_steps, d) and its timesteps
  float* temb1 = nullptr;        // (d,) time embedding of a scalar-t evaluation
  Grow<float> ffn_part;    // partial Y tiles of the small-M split FFN
  Grow<int> lstm_prog;     // progress words of the LSTM layer wavefront
  Grow<float> lstm_state;  // (tile, layer) state blocks of the time-chunked wavefront
  std::vector<float> ts_host;
  long weight_epoch = 0, temb_epoch = -1;
  // in-situ kernel timing (ffd_kernel_timing_*)
  uint32_t time_mask = 0;
  std::vector<hipEvent_t> ev;  // pairs (start, stop)
  std::vector<int> ev_cls;     // kernel class of each used pair
  size_t ev_used = 0;
  float tm_ms[FFD_K_COUNT] = {0};
  int tm_n[FFD_K_COUNT] = {0};
  int* async_err = nullptr;  // host-mapped word a kernel's timed-out wait writes (k_lstm_wave); read by check_async
  unsigned long long* lstm_trace = nullptr;  // ffd_lstm_trace: per-unit records of the next k_lstm_wave launch
  int lstm_trace_units = 0;
  // FreSca (sampler-level)
  bool fresca_on = false;
  bool crf_cap_on = false;
  ffd_crf_capture_cfg crf_cap{};
  ffd_fresca_cfg fcfg{};
  Grow<float> score2, fwork;
  // class conditioning / classifier-free guidance (ffd_class_enable): the table and the labels stay the caller's
  bool class_on = false;
  ffd_class_cfg ccls{};
  Grow<float> cls_temb, cls_x;  // (B | 2 B, d) embedding rows of one evaluation; the stacked batch (2 B, L, C)
  Grow<float> sm_noisy;  // the perturbed batch of ffd_sm_eval_batch
  Grow<float> ode_xp, ode_d1;  // Heun's predicted state and predictor drift (ffd_sample_batch_ode)
  Grow<float> ode_hist;        // the multistep solvers' history quantity q of the previous interval
  // whose history ode_hist holds: the solver and batch of the multistep call that ran last and the interval it ended at
  // (ms_solver < 0: none; every other loop entry drops it)
  int ms_solver = -1, ms_B = 0, ms_next = 0;
  Grow<float> lv_work;  // the Langevin corrector's row squares, norms and step sizes (ffd_sample_batch_pc)
  Grow<float> guide;  // ffd_sample_batch_guided: u, v and J^T v, one (B, L, C) slab each
  Grow<float> ll_stack, ll_v1;  // ffd_loglik_batch: the stacked batch of (1 + 2 k) B rows; Heun's v1 (B doubles)
  int tail_solver = FFD_SOLVER_EULER_MARUYAMA;  // the loop entry that ran last (ffd_kernel_work names its FFD_K_SDE tail)
  // CU partitions (ffd_tune "partitions"; run_partitioned): two streams confined to disjoint halves of the CUs, one fork
  // event and a join event per half, made on first use
  hipStream_t part_stream[2] = {nullptr, nullptr};
  hipEvent_t part_fork = nullptr, part_join[2] = {nullptr, nullptr};
  int part_budget = 0;  // CUs per partition; 0: not made yet, -1: this device's CUs cannot be halved that way
  int last_parts = 1;   // partitions the last sampling loop ran as (ffd_partition_status)
  // cache
  bool cache_enabled = false;
  ffd_cache_cfg ccfg{5, 10};
  float *kt = nullptr, *vt = nullptr;
  bool table_allocated = false;
  ffd_cache_stats stats{};

  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
  int d() const { return desc.d_model; }
  int hd() const { return desc.d_model / desc.n_head; }
  bool packs_made() const { return !layers.empty() && layers[0].in_wp != nullptr; }  // (transformer) by ffd_finalize_weights
  size_t table_floats() const { return (size_t)desc.num_layers * desc.n_head * desc.max_len * hd(); }
};

#define HIPCHECK(expr)                                                                          \
  do {                                                                                          \
    hipError_t e__ = (expr);                                                                    \
    if (e__ != hipSuccess)                                                                      \
      return ctx->fail(FFD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

namespace ffd {
#define FFD_KNOB_DEF(key, var, def, ...) thread_local int var = def;
FFD_KNOBS(FFD_KNOB_DEF, FFD_KNOB_DEF)
#undef FFD_KNOB_DEF
}  // namespace ffd

// n elements of 4 bytes (float; int for the LSTM progress words)
template <typename T>
static int dev_alloc(ffd_ctx* ctx, T** p, size_t n) {
  static_assert(sizeof(T) == sizeof(float), "the sizes in the messages are in floats");
  *p = nullptr;
  if (g_fail_alloc_after > 0 && --g_fail_alloc_after == 0)
    return ctx->fail(FFD_ERR_NOMEM, "hipMalloc(%zu floats) failed: injected by ffd_tune(\"fail_alloc_after\")", n);
  hipError_t e = hipMalloc((void**)p, n * sizeof(T) + 256);
  if (e != hipSuccess) return ctx->fail(FFD_ERR_NOMEM, "hipMalloc(%zu floats) failed: %s", n, hipGetErrorString(e));
  ctx->owned.push_back(*p);
  return FFD_OK;
}

// Make a workspace buffer hold at least n elements (contents are not kept).  The old allocation is released after the
// stream has drained (workspaces grow a handful of times; without this every growth kept the old buffer until
// ffd_destroy -- 3.6 GB for the q/k/v regions at B = 8192, L = 512).  The capacity reads 0 from the moment the old buffer
// is gone until the new one exists, so a failed growth (out of memory) leaves "nothing allocated", never a capacity that
// vouches for a freed or null pointer.
template <typename T>
static int ensure(ffd_ctx* ctx, Grow<T>& b, size_t n) {
  if (n <= b.cap) return FFD_OK;
  T* old = b.p;
  b.cap = 0;
  b.p = nullptr;
  if (old) {
    (void)hipDeviceSynchronize();
    auto it = std::find(ctx->owned.begin(), ctx->owned.end(), (void*)old);
    if (it != ctx->owned.end()) ctx->owned.erase(it);
    (void)hipFree(old);
  }
  int rc = dev_alloc(ctx, &b.p, n);
  if (rc == FFD_OK) b.cap = n;
  return rc;
}

// HIP event pair around a launch of kernel class `cls` while ffd_kernel_timing_begin has its bit set
struct Timed {
  ffd_ctx* ctx;
  hipStream_t s;
  bool on;
  Timed(ffd_ctx* c, int cls, hipStream_t st) : ctx(c), s(st) {
    on = ((c->time_mask >> cls) & 1u) && c->ev_used + 2 <= c->ev.size();
    if (on) {
      (void)hipEventRecord(c->ev[c->ev_used], s);
      c->ev_cls.push_back(cls);
    }
  }
  ~Timed() {
    if (on) {
      (void)hipEventRecord(ctx->ev[ctx->ev_used + 1], s);
      ctx->ev_used += 2;
    }
  }
};
#define TIMED(cls, expr)      \
  do {                        \
    Timed tm__(ctx, cls, s);  \
    HIPCHECK(expr);           \
  } while (0)

static bool d_supported(int d) {
#define X(v) if (d == v) return true;
  FFD_D_LIST(X)
#undef X
  return false;
}
static bool hd_supported(int hd) {
#define X(v) if (hd == v) return true;
  FFD_HD_LIST(X)
#undef X
  return false;
}

// ---------------------------------------------------------------------------
// kernel plan: which forms run a layer at this batch (declared in ffd_internal.h)
// ---------------------------------------------------------------------------
namespace ffd {

CacheMode cache_mode(int n_rec, int L) {
  if (n_rec < 0) return CACHE_STD;
  if (n_rec == L) return CACHE_FULL;
  if ((double)n_rec > 0.8 * (double)L) return CACHE_STD;
  return n_rec == 0 ? CACHE_PURE : CACHE_MIXED;
}

LayerPlan plan_layer(const ffd_model_desc& m, int B, CacheMode mode, const PackSet& pk) {
  const int L = m.max_len, d = m.d_model, H = m.n_head, hd = d / H, F = m.dim_feedforward, M = B * L;
  LayerPlan p{};
  // attention: the fused in-projection + attention kernel where one exists; at small batches its split form (the kv | q
  // pack where there is one and the step is not a pure cache hit), else one workgroup per head or head pair
  p.attn = g_attn_fused && pk.aw_full ? ATTN_FUSED : ATTN_TWO_KERNEL;
  p.hpw = 1;
  p.q_only = mode == CACHE_PURE;
  const int QT = cdiv(L, 32);
  if (p.attn == ATTN_FUSED) {
    p.kspl = qkv_attention_small_split(B, H, L);
    if (pk.aw_full2 && !p.kspl) p.hpw = qkv_attention_hpw(d, hd, L);
    if (g_attn_kvq && pk.aw_kvq && mode != CACHE_PURE && p.kspl) p.q_only = 2;
    // q-tiles per wave: the split form has one; a wave pair of the two-heads form takes half the q-tiles; attn_qg = 1 / 2
    // forces the instances of the full pack only (the q-only ones ignore it, and 3 means the heuristic here)
    p.qg = p.kspl                                               ? 1
           : p.hpw == 2                                         ? cdiv(QT, 2)
           : !p.q_only && (g_attn_qg == 1 || g_attn_qg == 2)    ? g_attn_qg
                                                                : attn_qg(QT, hd, true);
    // without the per-launch score bound where the layer's weights give it -- unless the launch reads K/V tables, whose
    // rows are projections of another step's hidden state
    p.attn_static = g_attn_static_bound && (mode == CACHE_STD || mode == CACHE_FULL);
  } else {
    p.qg = QT == 1 ? 1 : g_attn_qg ? g_attn_qg : attn_qg(QT, hd, false);
  }
  // FFN, in order of precedence: the opt-in bf16 split at every size; one 32- / 48-row k_ffn_ln tile per CU where the
  // 16-row tiles are 1.4 - 3 per CU (ahead of the small-M pair unless small_wgs is set, of the sliced k_ffn_rows unless
  // rows_slices is, and of the 64-row F slices unless mid_path forces them); the small-M F-split pair; the sliced
  // k_ffn_rows; the 64-row F slices; k_ffn_rows (out-projection inside where fused); k_ffn_ln
  const int hp = g_ffn_height && !g_ffn_split && !g_ffn_mb_override ? ffn_height_plan(M, d, F) : 0;
  int unf = 0;
  auto rows_nw = [&] { return g_ffn_rows_nw ? g_ffn_rows_nw : rows_waves(M); };  // unsliced k_ffn_rows: waves per workgroup
  if (g_ffn_split) {
    p.ffn = FFN_SPLIT;
  } else if (hp && g_ffn_height == 1) {
    p.ffn = FFN_LN_OPROJ, p.mb = hp;
  } else if (!(hp && g_small_wgs == 0) && (p.ns = small_path_splits(M, d, F))) {
    p.ffn = FFN_SMALL, p.part_floats = small_path_partial_floats(M, d, p.ns);
  } else if (pk.ring && !(hp && g_rows_slices == 0) && rows_slice_plan(M, d, F, &p.nw, &p.nslice, &unf)) {
    p.ffn = unf ? FFN_ROWS_SLICED : FFN_ROWS_SLICED_OPROJ, p.cps = 2, p.part_floats = rows_slice_floats(M, d, p.nslice);
  } else if ((p.nm = hp && g_mid_path == 1 ? 0 : mid_path_splits(M, d, F))) {
    p.ffn = FFN_MID, p.part_floats = small_path_partial_floats(cdiv(M, 64) * 64, d, p.nm);
  } else if (pk.ring && ffn_rows_fused_selected(M, d, F)) {
    p.ffn = FFN_ROWS_OPROJ, p.nw = rows_nw(), p.cps = 2;
  } else if (pk.ring && ffn_rows_selected(M, d, F)) {
    p.ffn = FFN_ROWS, p.nw = rows_nw(), p.cps = g_ffn_rows_cps == 1 && d == 72 ? 1 : 2;  // (one-chunk slots: d_model 72 only)
  } else {
    // k_ffn_ln tiles of 16 MB rows: MB = 4 (two workgroups resident per CU) once the grid fills the chip, smaller tiles
    // for smaller M; ffn_height = 2 puts the 32- / 48-row tiles behind k_linear_res_ln
    p.ffn = FFN_LN;
    p.mb = g_ffn_mb_override >= 1 ? g_ffn_mb_override : cdiv(M, 64) >= 512 ? 4 : cdiv(M, 32) >= 512 ? 2 : 1;
    if (hp) p.mb = hp;
    p.persist = g_ffn_persist;
  }
  if (p.ffn == FFN_LN || p.ffn == FFN_LN_OPROJ) p.rem = g_ffn_rem && ffn_rem_rows(d, p.mb);
  p.oproj_separate = p.ffn >= FFN_ROWS_SLICED;
  p.swap = p.ffn == FFN_ROWS_SLICED_OPROJ || p.ffn == FFN_ROWS_OPROJ;
  return p;
}

LstmPlan plan_lstm(const ffd_model_desc& m, int B) {
  // the layers as a wavefront (ffd_lstm.hip) in sub-batches of a 16-sample tile per CU; else the per-layer kernels
  const int maxb = lstm_wave_max_batch(m.max_len, m.d_model);
  if (g_lstm_wave && m.d_model % 4 == 0 && m.d_model >= 16 && m.num_layers <= 64 && maxb >= 16)
    return {true, B < maxb ? B : maxb};
  return {false, B};
}

}  // namespace ffd

extern "C" {

int ffd_tune(const char* key, int value) {
  if (!key) return FFD_ERR_INVALID;
  if (!strcmp(key, "reset")) {  // every knob back to its default (the test suite calls this after each test)
#define FFD_KNOB_RESET(k, var, def, ...) var = def;
    FFD_KNOBS(FFD_KNOB_RESET, FFD_KNOB_RESET)
#undef FFD_KNOB_RESET
    return FFD_OK;
  }
  const int v = value;
#define FFD_KNOB_SET(k, var, def, ok) \
  if (!strcmp(key, k)) {              \
    if (!(ok)) return FFD_ERR_INVALID; \
    var = v;                          \
    return FFD_OK;                    \
  }
#define FFD_KNOB_SET_BOOL(k, var, def) \
  if (!strcmp(key, k)) {               \
    var = v ? 1 : 0;                   \
    return FFD_OK;                     \
  }
  FFD_KNOBS(FFD_KNOB_SET, FFD_KNOB_SET_BOOL)
#undef FFD_KNOB_SET
#undef FFD_KNOB_SET_BOOL
  return FFD_ERR_INVALID;
}

int ffd_tune_get(const char* key, int* value) {
  if (!key || !value) return FFD_ERR_INVALID;
#define FFD_KNOB_GET(k, var, ...) \
  if (!strcmp(key, k)) {          \
    *value = var;                 \
    return FFD_OK;                \
  }
  FFD_KNOBS(FFD_KNOB_GET, FFD_KNOB_GET)  // (the calling thread's copy: the knobs are thread_local)
#undef FFD_KNOB_GET
  return FFD_ERR_INVALID;
}

const char* ffd_version(void) { return "libffd 0.1 (gfx950, fp32 MFMA 16x16x4, wave64)"; }

const char* ffd_last_error(const ffd_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ffd_host_noise_scaling(int max_len, int fourier_noise_scaling, float* G) {
  if (max_len < 1 || !G) return FFD_ERR_INVALID;
  // sde.py:49-58 in fp32: ones * (1/sqrt2); G[0] *= sqrt2; (even L) G[L/2] *= sqrt2
  for (int i = 0; i < max_len; ++i) G[i] = 1.0f;
  if (fourier_noise_scaling) {
    const float c = (float)(1.0 / sqrt(2.0));
    const float s2 = (float)sqrt(2.0);
    for (int i = 0; i < max_len; ++i) G[i] = c * G[i];
    G[0] = G[0] * s2;
    if (max_len % 2 == 0) G[max_len / 2] = G[max_len / 2] * s2;
  }
  return FFD_OK;
}

int ffd_host_timesteps(int n, double eps, float* ts, float* step_size) {
  if (n < 2 || !ts) return FFD_ERR_INVALID;
  // torch.linspace(1.0, eps, n) fp32 (scalar form of ATen's linspace kernel):
  // step = (end - start)/(n-1); idx < n/2 ? start + step*idx : end - step*(n-idx-1)
  const float start = 1.0f, end = (float)eps;
  const float step = (end - start) / (float)(n - 1);
  const int half = n / 2;
  for (int i = 0; i < n; ++i) {
    volatile float prod = (i < half) ? step * (float)i : step * (float)(n - i - 1);
    ts[i] = (i < half) ? start + prod : end - prod;
  }
  if (step_size) *step_size = ts[0] - ts[1];
  return FFD_OK;
}

int ffd_host_gate(int step, int max_len, int K, int R) {
  // caching.py:131-181
  if (step == 0) return max_len;
  const int interval = (R < 100) ? 500 : R;
  const int k_tokens = K < max_len ? K : max_len;
  if (step % interval == 0) {
    int n = 2 * k_tokens;
    if (n > max_len) n = max_len;
    return n < 0 ? 0 : n;
  }
  return 0;
}

// Upper bound of the largest eigenvalue of the symmetric n x n matrix a (row-major, overwritten): cyclic Jacobi sweeps
// until the off-diagonal part is negligible, then Gershgorin's bound max_i (a_ii + sum_j |a_ij|) of the rotated matrix.
// The rotations are similarity transforms, so that maximum bounds the largest eigenvalue from above however far the
// sweeps got (an iteration from below, such as the power method, could stop short of it); at convergence the
// off-diagonal sum is rounding noise and the bound is tight.  The relative 1e-12 covers the rotations' own rounding.
static double sym_eig_max_upper(std::vector<double>& a, int n) {
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) (i == j ? diag : off) += a[i * n + j] * a[i * n + j];
    if (off <= 1e-30 * diag) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[p * n + q];
        if (apq == 0.0) continue;
        const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < n; ++k) {  // A <- A J
          const double akp = a[k * n + p], akq = a[k * n + q];
          a[k * n + p] = c * akp - sn * akq, a[k * n + q] = sn * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {  // A <- J^T A
          const double apk = a[p * n + k], aqk = a[q * n + k];
          a[p * n + k] = c * apk - sn * aqk, a[q * n + k] = sn * apk + c * aqk;
        }
      }
  }
  double best = 0.0;
  for (int i = 0; i < n; ++i) {
    double r = a[i * n + i];
    for (int j = 0; j < n; ++j)
      if (j != i) r += fabs(a[i * n + j]);
    best = std::max(best, r);
  }
  return best * (1.0 + 1e-12);
}

int ffd_host_attn_score_bound(const float* in_w, const float* in_b, const float* ln_w, const float* ln_b, int d, int hd,
                              double q_scale, double* bound_out) {
  if (!in_w || !in_b || !ln_w || !ln_b || !bound_out || d < 1 || hd < 1 || d % hd != 0) return FFD_ERR_INVALID;
  // |LayerNorm(v)| <= sqrt(d) max|gamma| + |beta|: the normalised row has squared norm d var / (var + eps) <= d.  The
  // kernels' LayerNorm is fp32 (mean, variance, rsqrt, one FMA per element: a few ulp each); the relative 1e-4 is three
  // orders of magnitude above that and also covers the fp32 rounding of the projections that follow.
  constexpr double kLnSlack = 1e-4;
  double gmax = 0.0, b2 = 0.0;
  for (int i = 0; i < d; ++i) gmax = std::max(gmax, fabs((double)ln_w[i])), b2 += (double)ln_b[i] * ln_b[i];
  const double R = (sqrt((double)d) * gmax + sqrt(b2)) * (1.0 + kLnSlack);
  std::vector<double> gram((size_t)hd * hd);
  // sigma(W) R + |b| >= |W x + b| for |x| <= R, with sigma(W)^2 the largest eigenvalue of the head's Gram matrix W W^T
  auto reach = [&](int row0) {
    for (int i = 0; i < hd; ++i)
      for (int j = 0; j < hd; ++j) {
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc += (double)in_w[(size_t)(row0 + i) * d + k] * in_w[(size_t)(row0 + j) * d + k];
        gram[(size_t)i * hd + j] = acc;
      }
    double bb = 0.0;
    for (int i = 0; i < hd; ++i) bb += (double)in_b[row0 + i] * in_b[row0 + i];
    return sqrt(sym_eig_max_upper(gram, hd)) * R + sqrt(bb);
  };
  for (int h = 0; h < d / hd; ++h) bound_out[h] = q_scale * reach(h * hd) * reach(d + h * hd);
  return FFD_OK;
}

// ---------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------
// Every parameter of the state dict, in the order ffd_finalize_weights reports a missing one, bound to the field the
// launch sites read.  The one place that spells the keys.  (Runs before ffd_create has checked the shape.)
int ffd_host_cu_masks(int n_cus, int n_xcds, int layout, int parts, uint32_t* masks_out) {
  if (!masks_out || n_cus < 1 || n_xcds < 1 || parts < 1 || n_cus % n_xcds != 0) return FFD_ERR_INVALID;
  const int per_xcd = n_cus / n_xcds, words = (n_cus + 31) / 32;
  if (layout == FFD_CU_LAYOUT_SPREAD ? per_xcd % parts != 0 : layout == FFD_CU_LAYOUT_XCD ? n_xcds % parts != 0 : true)
    return FFD_ERR_INVALID;
  for (int i = 0; i < parts * words; ++i) masks_out[i] = 0u;
  for (int b = 0; b < n_cus; ++b) {  // mask bit b: CU b / n_xcds of XCD b % n_xcds
    const int part = layout == FFD_CU_LAYOUT_SPREAD ? (b / n_xcds) / (per_xcd / parts) : (b % n_xcds) / (n_xcds / parts);
    masks_out[part * words + b / 32] |= 1u << (b % 32);
  }
  return FFD_OK;
}

int ffd_partition_status(const ffd_ctx* ctx, int* parts_out) {
  if (!ctx || !parts_out) return FFD_ERR_INVALID;
  *parts_out = ctx->last_parts;
  return FFD_OK;
}

static void bind_weights(ffd_ctx* ctx) {
  const ffd_model_desc& m = ctx->desc;
  const int NL = std::max(m.num_layers, 0);
  const size_t d = m.d_model, C = m.n_channels, L = m.max_len, F = m.dim_feedforward;
  auto bind = [&](const std::string& key, size_t n, const float** field) { ctx->weights.push_back({key, n, field}); };
  ModelWeights& w = ctx->model;
  if (m.kind == FFD_MODEL_MIXTURE) {  // no network: the three tensors of the mixture (dim_feedforward carries K)
    const size_t K = std::max(m.dim_feedforward, 0);
    bind("mixture.means", K * L * C, &ctx->mix.means);
    bind("mixture.log_weights", K, &ctx->mix.logw);
    bind("mixture.variance", L * C, &ctx->mix.var);
    return;
  }
  if (m.kind == FFD_MODEL_TRANSFORMER) bind("pos_encoder.embedding.weight", L * d, &w.pos);
  bind("time_encoder.W", (d + 1) / 2, &w.time_W);
  bind("time_encoder.dense.weight", d * d, &w.time_dense_w);
  bind("time_encoder.dense.bias", d, &w.time_dense_b);
  const size_t io = m.kind == FFD_MODEL_MLP ? L * C : C;  // the MLP embeds the flattened series (score_models.py:392-397)
  bind("embedder.weight", d * io, &w.embed_w);
  bind("embedder.bias", d, &w.embed_b);
  bind("unembedder.weight", io * d, &w.unembed_w);
  bind("unembedder.bias", io, &w.unembed_b);
  if (m.kind == FFD_MODEL_TRANSFORMER) ctx->layers.resize(NL);
  else if (m.kind == FFD_MODEL_MLP) ctx->mlp.resize(NL);
  else ctx->lstm.resize(NL);
  for (int i = 0; i < NL; ++i) {
    const std::string s = (m.kind == FFD_MODEL_TRANSFORMER ? "backbone.layers." : "backbone.") + std::to_string(i) + ".";
    if (m.kind == FFD_MODEL_TRANSFORMER) {
      LayerWeights& l = ctx->layers[i];
      bind(s + "self_attn.in_proj_weight", 3 * d * d, &l.in_w);
      bind(s + "self_attn.in_proj_bias", 3 * d, &l.in_b);
      bind(s + "self_attn.out_proj.weight", d * d, &l.out_w);
      bind(s + "self_attn.out_proj.bias", d, &l.out_b);
      bind(s + "linear1.weight", F * d, &l.w1);
      bind(s + "linear1.bias", F, &l.b1);
      bind(s + "linear2.weight", d * F, &l.w2);
      bind(s + "linear2.bias", d, &l.b2);
      bind(s + "norm1.weight", d, &l.n1w);
      bind(s + "norm1.bias", d, &l.n1b);
      bind(s + "norm2.weight", d, &l.n2w);
      bind(s + "norm2.bias", d, &l.n2b);
    } else if (m.kind == FFD_MODEL_MLP) {
      MlpLayer& l = ctx->mlp[i];
      bind(s + "0.weight", F * d, &l.w0);
      bind(s + "0.bias", F, &l.b0);
      bind(s + "3.weight", d * F, &l.w3);
      bind(s + "3.bias", d, &l.b3);
    } else {
      LstmLayer& l = ctx->lstm[i];
      bind(s + "weight_ih_l0", 4 * d * d, &l.wih);
      bind(s + "weight_hh_l0", 4 * d * d, &l.whh);
      bind(s + "bias_ih_l0", 4 * d, &l.bih);
      bind(s + "bias_hh_l0", 4 * d, &l.bhh);
    }
  }
}

int ffd_create(ffd_ctx** out, const ffd_model_desc* desc, int device) {
  if (!out || !desc) return FFD_ERR_INVALID;
  *out = nullptr;
  ffd_ctx* ctx = new ffd_ctx();
  ctx->desc = *desc;
  ctx->device = device;
  *out = ctx;  // returned even on failure so the caller can read the message
  // the mixture kind has no network: d_model / n_head / num_layers are ignored.  Its "time embedding" is the time
  // itself, one float per evaluation, so every table and stride the loops size by d_model holds times (d_model = 1).
  if (ctx->desc.kind == FFD_MODEL_MIXTURE) ctx->desc.d_model = 1, ctx->desc.n_head = 1, ctx->desc.num_layers = 1;
  const ffd_model_desc& m = ctx->desc;
  bind_weights(ctx);
  if (m.n_channels < 1 || m.max_len < 1 || m.num_layers < 1)
    return ctx->fail(FFD_ERR_INVALID, "bad shape: C=%d L=%d NL=%d", m.n_channels, m.max_len, m.num_layers);
  if (m.kind == FFD_MODEL_MIXTURE) {
    if (m.dim_feedforward < 1) return ctx->fail(FFD_ERR_INVALID, "mixture: K=%d components", m.dim_feedforward);
    if (!mixture_shape_supported(1, m.dim_feedforward, m.max_len, m.n_channels))
      return ctx->fail(FFD_ERR_UNSUPPORTED, "mixture: L * C = %lld (limit %d), K = %d: no kernel for this shape",
                       (long long)m.max_len * m.n_channels, MIX_MAX_DIM, m.dim_feedforward);
  } else if (m.kind == FFD_MODEL_MLP) {
    if (m.d_model < 1 || m.dim_feedforward < 1)
      return ctx->fail(FFD_ERR_INVALID, "mlp: d_model=%d d_mlp=%d", m.d_model, m.dim_feedforward);
  } else if (!d_supported(m.d_model)) {
    return ctx->fail(FFD_ERR_UNSUPPORTED, "d_model=%d: this build has kernels for d_model in {8, 16, 24, 32, 48, 60, 64, 72}", m.d_model);
  }
  if (m.kind == FFD_MODEL_TRANSFORMER) {
    if (m.n_head < 1 || m.d_model % m.n_head != 0)
      return ctx->fail(FFD_ERR_INVALID, "d_model=%d not divisible by n_head=%d", m.d_model, m.n_head);
    if (!hd_supported(m.d_model / m.n_head))
      return ctx->fail(FFD_ERR_UNSUPPORTED, "head_dim=%d: supported head dims are 2, 3, 4, 5, 6, 8", m.d_model / m.n_head);
    if (m.dim_feedforward < 64 || m.dim_feedforward % 64 != 0)
      return ctx->fail(FFD_ERR_UNSUPPORTED, "dim_feedforward=%d must be a positive multiple of 64", m.dim_feedforward);
    if (m.max_len > 512) return ctx->fail(FFD_ERR_UNSUPPORTED, "max_len=%d > 512 (attention kernel limit)", m.max_len);
  } else if (m.kind != FFD_MODEL_LSTM && m.kind != FFD_MODEL_MLP && m.kind != FFD_MODEL_MIXTURE) {
    return ctx->fail(FFD_ERR_UNSUPPORTED, "model kind %d", m.kind);
  }
  if (m.sde != FFD_SDE_VP && m.sde != FFD_SDE_VE) return ctx->fail(FFD_ERR_UNSUPPORTED, "sde kind %d", m.sde);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return ctx->fail(FFD_ERR_HIP, "no HIP device available (%s): libffd has no CPU path",
                     e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return ctx->fail(FFD_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
  HIPCHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHECK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return ctx->fail(FFD_ERR_UNSUPPORTED, "device %d is %s; libffd is built for gfx950 only", device, prop.gcnArchName);
  ctx->G_host.resize(m.max_len);
  ffd_host_noise_scaling(m.max_len, m.fourier_noise_scaling, ctx->G_host.data());
  int rc = dev_alloc(ctx, &ctx->G_dev, m.max_len);
  if (rc) return rc;
  HIPCHECK(hipMemcpy(ctx->G_dev, ctx->G_host.data(), sizeof(float) * m.max_len, hipMemcpyHostToDevice));
  rc = dev_alloc(ctx, &ctx->temb1, m.d_model);
  if (rc) return rc;
  // (host memory the device writes through: readable by the host without a copy once the stream has drained)
  HIPCHECK(hipHostMalloc((void**)&ctx->async_err, 64, hipHostMallocMapped));
  memset(ctx->async_err, 0, 64);
  return FFD_OK;
}

void ffd_destroy(ffd_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (WeightSlot& w : ctx->weights) (void)hipFree(w.dev);
  for (void* p : ctx->owned) (void)hipFree(p);
  for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
  for (int p = 0; p < 2; ++p) {
    if (ctx->part_stream[p]) (void)hipStreamDestroy(ctx->part_stream[p]);
    if (ctx->part_join[p]) (void)hipEventDestroy(ctx->part_join[p]);
  }
  if (ctx->part_fork) (void)hipEventDestroy(ctx->part_fork);
  if (ctx->async_err) (void)hipHostFree(ctx->async_err);
  delete ctx;
}

int ffd_load_weight(ffd_ctx* ctx, const char* name, const float* data, size_t n) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!name || !data) return ctx->fail(FFD_ERR_INVALID, "ffd_load_weight: null argument");
  auto w = std::find_if(ctx->weights.begin(), ctx->weights.end(), [&](const WeightSlot& v) { return v.key == name; });
  if (w == ctx->weights.end()) return ctx->fail(FFD_ERR_INVALID, "unexpected parameter '%s' for this model", name);
  if (w->n != n) return ctx->fail(FFD_ERR_INVALID, "parameter '%s': got %zu floats, expected %zu", name, n, w->n);
  HIPCHECK(hipSetDevice(ctx->device));
  if (!w->dev) {
    hipError_t e = hipMalloc((void**)&w->dev, n * sizeof(float) + 256);
    if (e != hipSuccess) return ctx->fail(FFD_ERR_NOMEM, "hipMalloc for '%s' failed: %s", name, hipGetErrorString(e));
    *w->field = w->dev;
  }
  HIPCHECK(hipMemcpy(w->dev, data, n * sizeof(float), hipMemcpyDefault));
  ctx->finalized = false;
  return FFD_OK;
}

int ffd_finalize_weights(ffd_ctx* ctx) {
  if (!ctx) return FFD_ERR_INVALID;
  const ffd_model_desc& m = ctx->desc;
  for (const WeightSlot& w : ctx->weights)
    if (!w.dev)  // (the mixture's tensors are its definition, not a load order: a missing one is a bad argument)
      return ctx->fail(m.kind == FFD_MODEL_MIXTURE ? FFD_ERR_INVALID : FFD_ERR_STATE, "missing parameter '%s'", w.key.c_str());
  HIPCHECK(hipSetDevice(ctx->device));
  const int d = m.d_model, F = m.dim_feedforward;
  hipStream_t s = nullptr;
  if (m.kind == FFD_MODEL_MIXTURE) {
    // the values are checked once, on the host: a NaN mean or an all -inf weight vector would otherwise surface as NaN
    // samples many steps later
    const size_t D = (size_t)m.max_len * m.n_channels, K = m.dim_feedforward;
    std::vector<float> mu(K * D), lw(K), var(D);
    HIPCHECK(hipMemcpy(mu.data(), ctx->mix.means, mu.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(lw.data(), ctx->mix.logw, lw.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(var.data(), ctx->mix.var, var.size() * sizeof(float), hipMemcpyDeviceToHost));
    const char* why = "";
    if (int rc = mixture_check(mu.data(), lw.data(), var.data(), (int)K, m.max_len, m.n_channels, &why))
      return ctx->fail(rc, "mixture: %s", why);
  } else if (m.kind == FFD_MODEL_TRANSFORMER) {
    // (the one parameter the library writes: nn.Embedding(max_norm) renormalises its rows, transformer.py:13-15)
    HIPCHECK(launch_renorm_rows(const_cast<float*>(ctx->model.pos), m.max_len, d, sqrtf((float)d), s));
    for (LayerWeights& l : ctx->layers) {
      if (!l.in_wp) {  // first time: the packs
        int rc;
        if ((rc = dev_alloc(ctx, &l.in_wp, dpack_floats(3 * d, d)))) return rc;
        if ((rc = dev_alloc(ctx, &l.q_wp, dpack_floats(d, d)))) return rc;
        if ((rc = dev_alloc(ctx, &l.kv_wp, dpack_floats(2 * d, d)))) return rc;
        if (qkv_attention_supported(d, d / m.n_head)) {
          if ((rc = dev_alloc(ctx, &l.aw_full, attn_pack_floats(d, m.n_head, 1, 0)))) return rc;
          if ((rc = dev_alloc(ctx, &l.aw_q, attn_pack_floats(d, m.n_head, 1, 1)))) return rc;
          if (attn_kvq_supported(d / m.n_head))
            if ((rc = dev_alloc(ctx, &l.aw_kvq, attn_pack_floats(d, m.n_head, 1, 2)))) return rc;
          if (m.n_head % 2 == 0) {
            if ((rc = dev_alloc(ctx, &l.aw_full2, attn_pack_floats(d, m.n_head, 2, 0)))) return rc;
            if ((rc = dev_alloc(ctx, &l.aw_q2, attn_pack_floats(d, m.n_head, 2, 1)))) return rc;
          }
        }
        if ((rc = dev_alloc(ctx, &l.out_wp, dpack_floats(d, d)))) return rc;
        if ((rc = dev_alloc(ctx, &l.w1p, dpack_floats(F, d)))) return rc;
        if ((rc = dev_alloc(ctx, &l.w2p, w2pack_floats(d, F)))) return rc;
        if ((rc = dev_alloc(ctx, &l.w2r, w2rem_floats(d, F)))) return rc;
        if (ffn_rows_supported(d, F)) {
          if ((rc = dev_alloc(ctx, &l.ring, ffn_ring_floats(d, F)))) return rc;
          if ((rc = dev_alloc(ctx, &l.ring_op, ffn_ring_oproj_floats(d)))) return rc;
        }
      }
      HIPCHECK(launch_pack_dweight(l.in_w, l.in_wp, 3 * d, d, s));
      HIPCHECK(launch_pack_dweight(l.in_w, l.q_wp, d, d, s));
      HIPCHECK(launch_pack_dweight(l.in_w + (size_t)d * d, l.kv_wp, 2 * d, d, s));
      if (l.aw_full) {
        HIPCHECK(launch_pack_attn(l.in_w, l.in_b, l.aw_full, d, m.n_head, 1, 0, s));
        HIPCHECK(launch_pack_attn(l.in_w, l.in_b, l.aw_q, d, m.n_head, 1, 1, s));
        if (l.aw_kvq) HIPCHECK(launch_pack_attn(l.in_w, l.in_b, l.aw_kvq, d, m.n_head, 1, 2, s));
        if (l.aw_full2) {
          HIPCHECK(launch_pack_attn(l.in_w, l.in_b, l.aw_full2, d, m.n_head, 2, 0, s));
          HIPCHECK(launch_pack_attn(l.in_w, l.in_b, l.aw_q2, d, m.n_head, 2, 1, s));
        }
      }
      HIPCHECK(launch_pack_dweight(l.out_w, l.out_wp, d, d, s));
      HIPCHECK(launch_pack_dweight(l.w1, l.w1p, F, d, s));
      HIPCHECK(launch_pack_w2(l.w2, l.w2p, d, F, s));
      HIPCHECK(launch_pack_w2rem(l.w2, l.w2r, d, F, s));
      if (l.ring) {
        HIPCHECK(launch_pack_ffn_ring(l.w1, l.b1, l.w2, l.ring, d, F, s));
        HIPCHECK(launch_pack_oproj_ring(l.out_w, l.ring_op, d, s));
      }
      if (l.w1s) HIPCHECK(launch_pack_ffn_split(l.w1, l.w2, l.w1s, l.w2s, d, F, s));
    }
    // which layers' attention scores are bounded by the weights alone: the input of layer i >= 1 is layer i - 1's norm2
    // output (layer 0 reads the embedding of unbounded data and keeps measuring)
    const int hd = d / m.n_head;
    std::vector<float> in_w((size_t)3 * d * d), in_b(3 * d), g(d), be(d);
    std::vector<double> bound(m.n_head);
    for (size_t i = 0; i < ctx->layers.size(); ++i) {
      LayerWeights& l = ctx->layers[i];
      l.attn_bounded = false;
      if (i == 0 || !l.aw_full) continue;
      HIPCHECK(hipMemcpy(in_w.data(), l.in_w, in_w.size() * sizeof(float), hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(in_b.data(), l.in_b, in_b.size() * sizeof(float), hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(g.data(), ctx->layers[i - 1].n2w, d * sizeof(float), hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(be.data(), ctx->layers[i - 1].n2b, d * sizeof(float), hipMemcpyDeviceToHost));
      if (ffd_host_attn_score_bound(in_w.data(), in_b.data(), g.data(), be.data(), d, hd, attn_q_scale(hd), bound.data()))
        continue;
      l.attn_bounded = true;
      for (double v : bound) l.attn_bounded = l.attn_bounded && v <= (double)ATTN_SCORE_T;  // (a NaN weight: not bounded)
    }
  } else if (m.kind == FFD_MODEL_LSTM) {
    for (LstmLayer& l : ctx->lstm) {
      if (!l.wih_p) {  // first time: the packs
        int rc;
        if ((rc = dev_alloc(ctx, &l.wih_p, dpack_floats(4 * d, d)))) return rc;
        if ((rc = dev_alloc(ctx, &l.bsum, 4 * d))) return rc;
        if (d % 4 == 0 && d >= 16) {
          if ((rc = dev_alloc(ctx, &l.ih_wpk, lstm_wave_wpack_floats(d)))) return rc;
          if ((rc = dev_alloc(ctx, &l.hh_wpk, lstm_wave_wpack_floats(d)))) return rc;
          if ((rc = dev_alloc(ctx, &l.b_wpk, lstm_wave_bpack_floats(d)))) return rc;
        }
      }
      HIPCHECK(launch_pack_dweight(l.wih, l.wih_p, 4 * d, d, s));
      hipLaunchKernelGGL(k_add_vec, dim3(cdiv(4 * d, 256)), dim3(256), 0, s, l.bih, l.bhh, l.bsum, 4 * d);
      HIPCHECK(hipGetLastError());
      if (l.ih_wpk) HIPCHECK(launch_pack_lstm_wave(l.wih, l.whh, l.bsum, l.ih_wpk, l.hh_wpk, l.b_wpk, d, s));
    }
  }
  HIPCHECK(hipStreamSynchronize(s));
  ctx->weight_epoch++;
  ctx->finalized = true;
  return FFD_OK;
}

// ---------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------
static int ensure_workspace(ffd_ctx* ctx, int B) {
  const ffd_model_desc& m = ctx->desc;
  const size_t M = (size_t)B * m.max_len, d = m.d_model;
  int rc;
  if (m.kind == FFD_MODEL_MIXTURE) {  // no hidden state: the score, the per-sample times and the slices' partials
    if ((rc = ensure(ctx, ctx->score, M * m.n_channels))) return rc;
    if ((rc = ensure(ctx, ctx->temb_b, (size_t)B))) return rc;
    return ensure(ctx, ctx->mix_work, mixture_work_floats(B, m.dim_feedforward, m.max_len, m.n_channels));
  }
  if ((rc = ensure(ctx, ctx->h0, M * d))) return rc;
  if ((rc = ensure(ctx, ctx->score, M * m.n_channels))) return rc;
  if ((rc = ensure(ctx, ctx->temb_b, (size_t)B * d))) return rc;
  if (m.kind == FFD_MODEL_MLP) {
    if ((rc = ensure(ctx, ctx->h1, (size_t)B * d))) return rc;                   // ping-pong of the (B, d) state
    if ((rc = ensure(ctx, ctx->qkv, (size_t)B * m.dim_feedforward))) return rc;  // hidden (B, d_mlp)
  } else if (m.kind == FFD_MODEL_TRANSFORMER) {
    if ((rc = ensure(ctx, ctx->h1, M * d))) return rc;
    if ((rc = ensure(ctx, ctx->attn, M * d))) return rc;
  }
  // (the head-major q/k/v regions of the two-kernel attention fallback and the LSTM gate pre-activations are
  //  allocated on first use: the default paths never touch them -- 3.6 GB at B = 8192, L = 512)
  return FFD_OK;
}

static LayerPlan plan_of(const ffd_ctx* ctx, int B, CacheMode mode) {
  const LayerWeights& w = ctx->layers[0];  // (every layer has the same shape and packs)
  return plan_layer(ctx->desc, B, mode,
                    PackSet{w.aw_full != nullptr, w.aw_full2 != nullptr, w.aw_kvq != nullptr, w.ring_op != nullptr});
}

// What a cached mode means for a layer's attention: tokens below n_own use the sample's own K/V rows; `tables`: the others
// read the layer's K/V tables; `store`: batch element 0's recomputed rows go back into them (caching.py:326-328)
struct CacheUse {
  int n_own;
  bool tables, store;
};
static CacheUse cache_use(CacheMode mode, int n_rec, int L) {
  return {mode == CACHE_PURE ? 0 : mode == CACHE_MIXED ? n_rec : L, mode == CACHE_PURE || mode == CACHE_MIXED,
          mode == CACHE_MIXED};
}

// The FFD_K_ATTN launch(es) of layer weights w as planned, x -> ctx->attn.  kt / vt: the layer's K/V tables to read
// (cached modes); kt_out / vt_out: where batch element 0's recomputed rows go (MIXED).  The two-kernel form needs
// ctx->qkv to hold 3 M d floats.
static hipError_t run_attention(const ffd_ctx* ctx, const LayerPlan& p, const LayerWeights& w, const float* x,
                                const float* kt, const float* vt, float* kt_out, float* vt_out, int B, int n_own,
                                hipStream_t s, unsigned long long* stamp = nullptr) {
  const ffd_model_desc& m = ctx->desc;
  const int L = m.max_len, d = m.d_model, H = m.n_head, hd = d / H;
  float* out = ctx->attn.p;
  if (p.attn == ATTN_FUSED) {
    // in-projection + attention in one launch: q/k/v never leave the CU (ffd_qkvattn.hip); in MIXED batch element 0's
    // workgroups also publish their recomputed K/V rows (caching.py:326-328)
    const float* pack = p.q_only == 2 ? w.aw_kvq
                        : p.hpw == 2  ? (p.q_only ? w.aw_q2 : w.aw_full2)
                                      : (p.q_only ? w.aw_q : w.aw_full);
    return launch_qkv_attention(AttnArgs{x, pack, kt, vt, kt_out, vt_out, out, B, L, n_own, stamp,
                                         p.attn_static && w.attn_bounded && kt == nullptr},
                                d, hd, p.hpw, p.q_only, p.kspl, p.qg, s);
  }
  if (stamp != nullptr) return hipErrorInvalidValue;
  // q / k / v regions, head-major (B,H,L,hd)
  const size_t M = (size_t)B * L;
  float *q = ctx->qkv.p, *k = q + M * d, *v = q + 2 * M * d;
  hipError_t e = launch_linear_hm(x, p.q_only ? w.q_wp : w.in_wp, w.in_b, q, k, v, (int)M, p.q_only ? 1 : 3, d, L, H, hd, s);
  if (e == hipSuccess) e = launch_attention(q, k, v, kt, vt, out, B, L, H, hd, n_own, p.qg, s);
  if (e == hipSuccess && kt_out)  // (caching.py:326-328, cached_transformer.py:301-305)
    e = launch_kv_store(k, v, kt_out, vt_out, L, H, hd, n_own, s);
  return e;
}

// The FFD_K_FFN launch(es) of layer weights w as planned: from attn + the residual rows cur, or (p.oproj_separate) from
// the k_linear_res_ln output in alt; the output goes to cur, or to alt where p.swap.  ctx->ffn_part holds p.part_floats.
static hipError_t run_ffn(const ffd_ctx* ctx, const LayerPlan& p, const LayerWeights& w, const float* attn, float* cur,
                          float* alt, int M, hipStream_t s, unsigned long long* stamp = nullptr) {
  const int d = ctx->desc.d_model, F = ctx->desc.dim_feedforward;
  float* P = ctx->ffn_part.p;
  // k_ffn_rows: whole rows (the fused form: x1 never leaves the CU; rows are read and written by different waves, so no
  // in-place form), or tiles x slices of the hidden dimension into P + the reduce / LN2 launch (slices added in order)
  const bool sliced = p.ffn == FFN_ROWS_SLICED_OPROJ || p.ffn == FFN_ROWS_SLICED;
  const bool fused = p.ffn == FFN_ROWS_SLICED_OPROJ || p.ffn == FFN_ROWS_OPROJ;
  float* const y = fused ? alt : cur;
  const RowsArgs rows{fused ? attn : alt, fused ? cur : nullptr, &w, sliced ? P : y, M, d, F, p.nw, p.cps, fused,
                      sliced ? p.nslice : 0, stamp};
  switch (p.ffn) {
    case FFN_LN_OPROJ:  // one 32- / 48-row tile per CU, out-proj + LN1 + FFN + LN2 in one launch, in place
      return stamp ? hipErrorInvalidValue : launch_oproj_ffn_ln(attn, cur, w, cur, M, d, F, p.mb, p.rem, s);
    case FFN_SMALL:  // out-proj + LN1 recomputed per F split, FFN partials + a deterministic reduce / LN2 launch
      return stamp ? hipErrorInvalidValue : launch_oproj_ffn_small(attn, cur, w, alt, P, cur, M, d, F, p.ns, s);
    case FFN_ROWS_SLICED_OPROJ:
    case FFN_ROWS_SLICED: {
      if (stamp || p.nslice < 2) return hipErrorInvalidValue;
      const hipError_t e = launch_ffn_rows(rows, s);
      return e != hipSuccess ? e : launch_rows_reduce_ln(P, w, y, M, d, p.nslice, s);
    }
    case FFN_ROWS_OPROJ:
    case FFN_ROWS: return launch_ffn_rows(rows, s);
    case FFN_MID:  // 64-row tiles x F slices, partial tiles + the reduce / LN2 launch
      return stamp ? hipErrorInvalidValue : launch_ffn_mid(alt, w, P, cur, M, d, F, p.nm, s);
    case FFN_SPLIT: return launch_ffn_ln_split(alt, w, cur, M, d, F, s, stamp);
    case FFN_LN: return launch_ffn_ln(alt, w, cur, M, d, F, p.mb, p.rem, p.persist, s, stamp);
  }
  return hipErrorInvalidValue;
}

// ffd_kernel_work's row per FFN form: name; the out-projection inside it (work of one, per slice where sliced)
static const struct {
  const char* name;
  bool oproj;
} kFfnForms[] = {
    {"k_ffn_ln<oproj>", true},                                  // FFN_LN_OPROJ
    {"k_oproj_ffn_split + k_ffn_reduce_ln", true},              // FFN_SMALL
    {"k_ffn_rows<oproj, sliced> + k_rows_reduce_ln", true},     // FFN_ROWS_SLICED_OPROJ
    {"k_ffn_rows<oproj>", true},                                // FFN_ROWS_OPROJ
    {"k_ffn_rows<sliced> + k_rows_reduce_ln", false},           // FFN_ROWS_SLICED
    {"k_ffn_part", false},                                      // FFN_MID
    {"k_ffn_ln_split", false},                                  // FFN_SPLIT
    {"k_ffn_rows", false},                                      // FFN_ROWS
    {"k_ffn_ln", false},                                        // FFN_LN
};

// one score evaluation; temb points at d floats on the device (temb_stride = 0: shared by the batch) or at a
// (B, d) table (temb_stride = d: per-sample diffusion times).
// n_rec < 0: no cache.  Otherwise the E2-CRF mode for |recompute_tokens| = n_rec.
// hidden_out != nullptr (transformer / LSTM): skip the unembedding and return the final hidden state (M x d) instead;
// the sampling loop unembeds inside the SDE-step kernel.
static int forward_impl(ffd_ctx* ctx, const float* x, const float* temb, int temb_stride, float* score_out,
                        float* crf_out, int B, int n_rec, hipStream_t s, const float** hidden_out = nullptr) {
  const ffd_model_desc& m = ctx->desc;
  const int L = m.max_len, C = m.n_channels, d = m.d_model, M = B * L;
  const ModelWeights& mw = ctx->model;
  if (m.kind == FFD_MODEL_MIXTURE) {
    // the closed-form score (ffd_mixture.hip): `temb` holds the evaluation's time(s) -- one float shared by the batch
    // (a row of the trajectory's table, which for this kind is the timestep grid itself) or one per sample
    TIMED(FFD_K_ATTN, launch_mixture_score(m.sde, m.sde_a, m.sde_b, x, temb, temb_stride ? 1 : 0, ctx->mix.means,
                                           ctx->mix.logw, ctx->mix.var, ctx->G_dev, score_out, B, m.dim_feedforward, L, C,
                                           ctx->mix_work.p, s));
    return FFD_OK;
  }
  if (m.kind == FFD_MODEL_MLP) {  // MLPScoreModule.forward, score_models.py:406-440
    const int io = L * C, F = m.dim_feedforward;
    // flatten "b t c -> b (t c)" is the memory layout already; time encoding is one (d,) vector per step
    // embedder(X) + time encoding: one (d,) vector per step (second bias), or a (B, d) table (added like a residual)
    HIPCHECK(launch_dense(x, mw.embed_w, mw.embed_b, temb_stride ? nullptr : temb, temb_stride ? temb : nullptr,
                          ctx->h0.p, B, d, io, 0, s));
    float* cur = ctx->h0.p;
    float* alt = ctx->h1.p;
    for (const MlpLayer& l : ctx->mlp) {
      HIPCHECK(launch_dense(cur, l.w0, l.b0, nullptr, nullptr, ctx->qkv.p, B, F, d, 1, s));
      HIPCHECK(launch_dense(ctx->qkv.p, l.w3, l.b3, nullptr, cur, alt, B, d, F, 0, s));  // X + layer(X)
      std::swap(cur, alt);
    }
    HIPCHECK(launch_dense(cur, mw.unembed_w, mw.unembed_b, nullptr, nullptr, score_out, B, io, d, 0, s));
    return FFD_OK;
  }
  float* const h0 = ctx->h0.p;
  if (m.kind == FFD_MODEL_LSTM) {
    TIMED(FFD_K_EMBED, launch_embed(x, mw.embed_w, mw.embed_b, nullptr, temb, temb_stride, h0, B, L, C, d, s));
    if (const LstmPlan lp = plan_lstm(m, B); lp.wave) {
      const int Bw = lp.Bw;  // samples per launch
      if (int rc = ensure(ctx, ctx->lstm_prog, (size_t)16 + 16 * cdiv(Bw, 16))) return rc;
      const float *wih[64], *whh[64], *bs[64];
      for (int i = 0; i < m.num_layers; ++i) wih[i] = ctx->lstm[i].ih_wpk, whh[i] = ctx->lstm[i].hh_wpk, bs[i] = ctx->lstm[i].b_wpk;
      if (int rc = ensure(ctx, ctx->lstm_state, lstm_wave_state_floats(Bw, d, m.num_layers))) return rc;
      for (int b0 = 0; b0 < B; b0 += Bw) {  // (samples are independent: sub-batches of a tile per CU, one after the other)
        const int nb = B - b0 < Bw ? B - b0 : Bw;
        TIMED(FFD_K_LSTM_REC, launch_lstm_wave(h0 + (size_t)b0 * L * d, wih, whh, bs, m.num_layers, nb, L, d,
                                               ctx->lstm_prog.p, ctx->lstm_state.p, ctx->async_err, s,
                                               b0 == 0 ? ctx->lstm_trace : nullptr));
      }
    } else
    for (const LstmLayer& l : ctx->lstm) {
      if (int rc = ensure(ctx, ctx->qkv, (size_t)M * 4 * d)) return rc;  // gate pre-activations gx
      TIMED(FFD_K_LSTM_GATES, launch_linear(h0, l.wih_p, l.bsum, ctx->qkv.p, M, 4 * d, d, 4 * d, s));
      TIMED(FFD_K_LSTM_REC, launch_lstm_layer(h0, ctx->qkv.p, l.whh, B, L, d, s));
    }
    if (hidden_out) {
      *hidden_out = h0;
      return FFD_OK;
    }
    TIMED(FFD_K_UNEMBED, launch_unembed(h0, mw.unembed_w, mw.unembed_b, score_out, M, C, d, s));
    return FFD_OK;
  }
  const int H = m.n_head, hd = d / H, F = m.dim_feedforward;
  TIMED(FFD_K_EMBED, launch_embed(x, mw.embed_w, mw.embed_b, mw.pos, temb, temb_stride, h0, B, L, C, d, s));
  const CacheMode mode = cache_mode(n_rec, L);  // cached_transformer.py:139-220
  const CacheUse cu = cache_use(mode, n_rec, L);
  const size_t lt = (size_t)H * L * hd;  // table floats per layer
  // opt-in: the FFN on the bf16 matrix cores as a three-part split (ffd_ffn_split.hip); takes every batch size, so
  // that all parity cases exercise it when it is on
  if (g_ffn_split && !ffn_split_supported(d, F))
    return ctx->fail(FFD_ERR_UNSUPPORTED, "ffn_split needs d_model %% 4 == 0, d_model <= 96, dim_feedforward %% 128 == 0");
  const LayerPlan plan = plan_of(ctx, B, mode);
  if (plan.attn == ATTN_TWO_KERNEL)
    if (int rc = ensure(ctx, ctx->qkv, (size_t)M * 3 * d)) return rc;
  if (int rc = ensure(ctx, ctx->ffn_part, plan.part_floats)) return rc;
  float* const attn = ctx->attn.p;
  float* cur = h0;  // layer input / residual
  float* alt = ctx->h1.p;
  for (int i = 0; i < m.num_layers; ++i) {
    LayerWeights& w = ctx->layers[i];
    float* kt = ctx->kt ? ctx->kt + i * lt : nullptr;
    float* vt = ctx->vt ? ctx->vt + i * lt : nullptr;
    TIMED(FFD_K_ATTN, run_attention(ctx, plan, w, cur, cu.tables ? kt : nullptr, cu.tables ? vt : nullptr,
                                    cu.store ? kt : nullptr, cu.store ? vt : nullptr, B, cu.n_own, s));
    if (plan.ffn == FFN_SPLIT && w.w1s == nullptr) {  // first use: make the packs
      if (int rc = dev_alloc(ctx, &w.w1s, w1split_bytes(d, F) / sizeof(float))) return rc;
      if (int rc = dev_alloc(ctx, &w.w2s, w2split_bytes(d, F) / sizeof(float))) return rc;
      HIPCHECK(launch_pack_ffn_split(w.w1, w.w2, w.w1s, w.w2s, d, F, s));
    }
    if (plan.oproj_separate)
      TIMED(FFD_K_OUTPROJ, launch_linear_res_ln(attn, w.out_wp, w.out_b, cur, w.n1w, w.n1b, alt, M, d, s));
    TIMED(FFD_K_FFN, run_ffn(ctx, plan, w, attn, cur, alt, M, s));
    if (plan.swap) std::swap(cur, alt);
    if (mode == CACHE_FULL) {
      // K,V of the layer OUTPUT for batch element 0 (cached_transformer.py:144-158), written
      // straight into this layer's tables: head-major (1,H,L,hd) == table layout
      HIPCHECK(launch_linear_hm(cur, w.kv_wp, w.in_b + d, kt, vt, nullptr, L, 2, d, L, H, hd, s));
    }
    if (n_rec >= 0 && crf_out)  // crf[l] = h_l[0]  (score_models.py:181-194)
      HIPCHECK(hipMemcpyAsync(crf_out + (size_t)i * L * d, cur, sizeof(float) * L * d, hipMemcpyDeviceToDevice, s));
  }
  if (n_rec >= 0) {  // counters, caching.py:283,299,396
    if (mode == CACHE_FULL) ctx->stats.recompute_count += (int64_t)L * m.num_layers, ctx->table_allocated = true;
    else if (mode == CACHE_PURE) ctx->stats.cache_hit_count += (int64_t)L * m.num_layers;
    else if (mode == CACHE_MIXED) {
      ctx->stats.cache_hit_count += (int64_t)(L - n_rec) * m.num_layers;
      ctx->stats.recompute_count += (int64_t)n_rec * m.num_layers;
      ctx->table_allocated = true;
    }
  }
  if (hidden_out) {
    *hidden_out = cur;
    return FFD_OK;
  }
  TIMED(FFD_K_UNEMBED, launch_unembed(cur, mw.unembed_w, mw.unembed_b, score_out, M, C, d, s));
  return FFD_OK;
}

// A kernel whose bounded wait ran out (k_lstm_wave's progress-word protocol) has left a code in ctx->async_err: the
// results of that launch are void.  Reported once, by whichever entry point comes next (or ffd_async_status).
static int check_async(ffd_ctx* ctx) {
  if (!ctx->async_err) return FFD_OK;
  const int code = *reinterpret_cast<volatile int*>(ctx->async_err);
  if (code == 0) return FFD_OK;
  *reinterpret_cast<volatile int*>(ctx->async_err) = 0;
  return ctx->fail(FFD_ERR_STATE,
                   "k_lstm_wave: unit %d waited longer than %d ms for the unit it depends on (the layer wavefront needs the "
                   "device's compute units to itself: another stream or process was holding some); the results of that "
                   "launch are invalid", code - 1, g_lstm_wave_spin_ms);
}

static int check_ready(ffd_ctx* ctx, int B) {
  if (int rc = check_async(ctx)) return rc;
  if (!ctx->finalized) return ctx->fail(FFD_ERR_STATE, "weights not finalised (call ffd_finalize_weights)");
  if (B < 1) return ctx->fail(FFD_ERR_INVALID, "batch size %d", B);
  if ((double)B * ctx->desc.max_len * 4 * ctx->desc.d_model > 2.0e9)
    return ctx->fail(FFD_ERR_UNSUPPORTED, "batch %d too large for 32-bit row indexing; shard the batch", B);
  if (ctx->desc.kind == FFD_MODEL_MIXTURE &&
      !mixture_shape_supported(B, ctx->desc.dim_feedforward, ctx->desc.max_len, ctx->desc.n_channels))
    return ctx->fail(FFD_ERR_UNSUPPORTED, "batch %d too large for the mixture kernel's indexing; shard the batch", B);
  return FFD_OK;
}

// Class conditioning (include/ffd.h ffd_class_enable): does an evaluation run the stacked batch of 2 B rows, what an
// entry that honours the state checks before anything else, and what the entries without a class form answer
static bool class_stacked(const ffd_ctx* ctx) {
  return ctx->class_on && ctx->ccls.guidance_scale != 1.f && ctx->ccls.guidance_scale != 0.f;
}
static int class_check(ffd_ctx* ctx, const char* who, int B, bool cached) {
  if (!ctx->class_on) return FFD_OK;
  if (cached)
    return ctx->fail(FFD_ERR_STATE, "%s: class conditioning is on (ffd_class_disable): the E2-CRF cache shares batch element "
                     "0's rows, which carry that sample's label", who);
  if (ctx->ccls.labels && ctx->ccls.n_labels != B)
    return ctx->fail(FFD_ERR_INVALID, "%s: %d labels for a batch of %d", who, ctx->ccls.n_labels, B);
  return FFD_OK;
}
static int class_refuse(ffd_ctx* ctx, const char* who) {
  if (!ctx->class_on) return FFD_OK;
  return ctx->fail(FFD_ERR_STATE, "%s has no class-conditional form: class conditioning is on (call ffd_class_disable)", who);
}
// per-sample embeddings (B, d) -> + table[label_b], in place (the conditional branch)
static int class_add_rows(ffd_ctx* ctx, float* temb, int B, hipStream_t s) {
  if (!ctx->class_on) return FFD_OK;
  const ffd_class_cfg& c = ctx->ccls;
  HIPCHECK(launch_class_temb(temb, ctx->desc.d_model, c.table, c.n_classes, c.labels, B, ctx->desc.d_model, 0, temb, nullptr,
                             nullptr, 0, s));
  return FFD_OK;
}

// temb[n][d] for the n timesteps ts on the device, or (ts == nullptr, n = 1) for the scalar t
static int time_embed(ffd_ctx* ctx, const float* ts, float t, int n, float* temb, hipStream_t s) {
  const ModelWeights& w = ctx->model;
  if (ctx->desc.kind == FFD_MODEL_MIXTURE) {  // the closed-form score reads the time itself
    HIPCHECK(launch_mixture_times(ts, t, n, temb, s));
    return FFD_OK;
  }
  HIPCHECK(launch_time_embed(ts, t, n, w.time_W, w.time_dense_w, w.time_dense_b, temb, ctx->desc.d_model, s));
  return FFD_OK;
}

// What the three ffd_score_forward* entry points do once their arguments have passed: one time embedding for the batch
// (ts == nullptr: the scalar t) or one per sample: dense(gamma(t_b)) (transformer.py:77-91)
static int score_forward(ffd_ctx* ctx, const float* x, const float* ts, float t, float* score_out, float* crf_out, int B,
                         int n_rec, void* stream) {
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = ensure_workspace(ctx, B)) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* temb = ts ? ctx->temb_b.p : ctx->temb1;
  if (int rc = time_embed(ctx, ts, ts ? 0.f : t, ts ? B : 1, temb, s)) return rc;
  if (ts)
    if (int rc = class_add_rows(ctx, temb, B, s)) return rc;
  return forward_impl(ctx, x, temb, ts ? ctx->desc.d_model : 0, score_out, crf_out, B, n_rec, s);
}

// (n_recompute's range is checked by the caller: the entry points differ in where it comes among their checks)
static int check_cached(ffd_ctx* ctx) {
  if (ctx->desc.kind != FFD_MODEL_TRANSFORMER)
    return ctx->fail(FFD_ERR_UNSUPPORTED, "caching is only defined for the transformer backbone (SURVEY Q9)");
  if (!ctx->cache_enabled) return ctx->fail(FFD_ERR_STATE, "cache not enabled (call ffd_cache_enable)");
  return FFD_OK;
}

int ffd_score_forward(ffd_ctx* ctx, const float* x, float t, float* score_out, int B, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (int rc = class_refuse(ctx, "ffd_score_forward (one time for the batch)")) return rc;
  if (int rc = check_ready(ctx, B)) return rc;
  if (!x || !score_out) return ctx->fail(FFD_ERR_INVALID, "null buffer");
  return score_forward(ctx, x, nullptr, t, score_out, nullptr, B, -1, stream);
}

int ffd_score_forward_cached(ffd_ctx* ctx, const float* x, float t, float* score_out, float* crf_out, int B,
                             int n_recompute, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (int rc = class_refuse(ctx, "ffd_score_forward_cached")) return rc;
  if (int rc = check_ready(ctx, B)) return rc;
  if (int rc = check_cached(ctx)) return rc;
  if (!x || !score_out) return ctx->fail(FFD_ERR_INVALID, "null buffer");
  if (n_recompute < 0 || n_recompute > ctx->desc.max_len)
    return ctx->fail(FFD_ERR_INVALID, "n_recompute=%d outside [0,%d]", n_recompute, ctx->desc.max_len);
  return score_forward(ctx, x, nullptr, t, score_out, crf_out, B, n_recompute, stream);
}

int ffd_score_forward_ts(ffd_ctx* ctx, const float* x, const float* timesteps, float* score_out, float* crf_out,
                         int B, int n_recompute, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (int rc = class_check(ctx, "ffd_score_forward_ts", B, n_recompute >= 0)) return rc;
  if (int rc = check_ready(ctx, B)) return rc;
  if (!x || !timesteps || !score_out) return ctx->fail(FFD_ERR_INVALID, "null buffer");
  if (n_recompute >= 0) {
    if (int rc = check_cached(ctx)) return rc;
    if (n_recompute > ctx->desc.max_len)
      return ctx->fail(FFD_ERR_INVALID, "n_recompute=%d outside [0,%d]", n_recompute, ctx->desc.max_len);
  }
  return score_forward(ctx, x, timesteps, 0.f, score_out, n_recompute >= 0 ? crf_out : nullptr, B,
                       n_recompute >= 0 ? n_recompute : -1, stream);
}

// loss_fn's body for one batch (losses.py:65-122): perturb -> score network at the per-sample times -> per-sample loss
int ffd_sm_eval_batch(ffd_ctx* ctx, const float* x0, const float* timesteps, const float* mean_coeff, const float* sigma,
                      const float* z, uint64_t seed, uint64_t sample_offset, int likelihood_weighting, int reduce_mean,
                      double* per_sample_out, int B, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (int rc = class_check(ctx, "ffd_sm_eval_batch", B, false)) return rc;
  if (int rc = check_ready(ctx, B)) return rc;
  if (!x0 || !timesteps || !mean_coeff || !sigma || !per_sample_out) return ctx->fail(FFD_ERR_INVALID, "null buffer");
  const ffd_model_desc& m = ctx->desc;
  const int L = m.max_len, C = m.n_channels;
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = ensure_workspace(ctx, B)) return rc;
  if (int rc = ensure(ctx, ctx->sm_noisy, (size_t)B * L * C)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHECK(launch_sm_perturb(x0, ctx->sm_noisy.p, mean_coeff, sigma, ctx->G_dev, z, seed, sample_offset, B, L, C, s));
  if (int rc = time_embed(ctx, timesteps, 0.f, B, ctx->temb_b.p, s)) return rc;
  if (int rc = class_add_rows(ctx, ctx->temb_b.p, B, s)) return rc;
  if (int rc = forward_impl(ctx, ctx->sm_noisy.p, ctx->temb_b.p, m.d_model, ctx->score.p, nullptr, B, -1, s)) return rc;
  HIPCHECK(launch_sm_loss(ctx->score.p, sigma, ctx->G_dev, z, seed, sample_offset, likelihood_weighting, reduce_mean,
                          per_sample_out, B, L, C, s));
  return FFD_OK;
}

int ffd_fresca_enable(ffd_ctx* ctx, const ffd_fresca_cfg* cfg) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!cfg) return ctx->fail(FFD_ERR_INVALID, "null fresca config");
  if (cfg->strategy != FFD_FRESCA_SPATIAL && cfg->strategy != FFD_FRESCA_ENERGY)
    return ctx->fail(FFD_ERR_INVALID, "unknown cutoff strategy %d", cfg->strategy);
  ctx->fcfg = *cfg;
  ctx->fresca_on = true;
  return FFD_OK;
}

int ffd_fresca_disable(ffd_ctx* ctx) {
  if (!ctx) return FFD_ERR_INVALID;
  ctx->fresca_on = false;
  return FFD_OK;
}

int ffd_class_enable(ffd_ctx* ctx, const ffd_class_cfg* cfg) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!cfg) return ctx->fail(FFD_ERR_INVALID, "null class config");
  if (ctx->desc.kind == FFD_MODEL_MIXTURE)
    return ctx->fail(FFD_ERR_UNSUPPORTED, "the mixture kind has no embedding to condition (its classes are its components)");
  if (!cfg->table || cfg->n_classes < 1) return ctx->fail(FFD_ERR_INVALID, "class config: table and n_classes >= 1 are required");
  if (!std::isfinite(cfg->guidance_scale)) return ctx->fail(FFD_ERR_INVALID, "guidance_scale must be finite");
  if (cfg->labels) {
    if (!cfg->labels_host || cfg->n_labels < 1)
      return ctx->fail(FFD_ERR_INVALID, "device labels need their host copy (labels_host) and n_labels >= 1");
    for (int i = 0; i < cfg->n_labels; ++i)
      if (cfg->labels_host[i] < -1 || cfg->labels_host[i] > cfg->n_classes)
        return ctx->fail(FFD_ERR_INVALID, "label %d of sample %d outside [-1, %d]", cfg->labels_host[i], i, cfg->n_classes);
  }
  ctx->ccls = *cfg;
  ctx->ccls.labels_host = nullptr;  // (validated, not kept)
  ctx->class_on = true;
  return FFD_OK;
}

int ffd_class_disable(ffd_ctx* ctx) {
  if (!ctx) return FFD_ERR_INVALID;
  ctx->class_on = false;
  return FFD_OK;
}

int ffd_cache_crf_capture(ffd_ctx* ctx, const ffd_crf_capture_cfg* cfg) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!cfg) {
    ctx->crf_cap_on = false;
    return FFD_OK;
  }
  if ((cfg->ring && (cfg->n_slots < 1 || cfg->every < 1)) || (cfg->last && cfg->last_every < 1))
    return ctx->fail(FFD_ERR_INVALID, "bad CRF capture config (n_slots=%d every=%d last_every=%d)", cfg->n_slots,
                     cfg->every, cfg->last_every);
  ctx->crf_cap = *cfg;
  ctx->crf_cap_on = cfg->ring || cfg->last;
  return FFD_OK;
}

// ---------------------------------------------------------------------------
// cache lifecycle
// ---------------------------------------------------------------------------
int ffd_cache_enable(ffd_ctx* ctx, const ffd_cache_cfg* cfg) {
  if (!ctx) return FFD_ERR_INVALID;
  if (ctx->desc.kind != FFD_MODEL_TRANSFORMER)
    return ctx->fail(FFD_ERR_UNSUPPORTED, "caching is only defined for the transformer backbone (SURVEY Q9)");
  HIPCHECK(hipSetDevice(ctx->device));
  if (cfg) ctx->ccfg = *cfg;
  if (!ctx->kt) {
    int rc;
    if ((rc = dev_alloc(ctx, &ctx->kt, ctx->table_floats()))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->vt, ctx->table_floats()))) return rc;
  }
  ctx->cache_enabled = true;
  return ffd_cache_reset(ctx);
}

int ffd_cache_configure(ffd_ctx* ctx, const ffd_cache_cfg* cfg) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!cfg) return ctx->fail(FFD_ERR_INVALID, "null cache config");
  if (!ctx->cache_enabled) return ctx->fail(FFD_ERR_STATE, "cache not enabled (call ffd_cache_enable)");
  ctx->ccfg = *cfg;
  return FFD_OK;
}

int ffd_cache_disable(ffd_ctx* ctx) {
  if (!ctx) return FFD_ERR_INVALID;
  ctx->cache_enabled = false;
  return FFD_OK;
}

int ffd_cache_reset(ffd_ctx* ctx) {
  if (!ctx) return FFD_ERR_INVALID;
  HIPCHECK(hipSetDevice(ctx->device));
  if (ctx->kt) {
    // an unallocated reference table reads as zeros (cached_transformer.py:252-257)
    HIPCHECK(hipMemset(ctx->kt, 0, ctx->table_floats() * sizeof(float)));
    HIPCHECK(hipMemset(ctx->vt, 0, ctx->table_floats() * sizeof(float)));
  }
  ctx->table_allocated = false;
  ctx->stats = ffd_cache_stats{};
  return FFD_OK;
}

int ffd_cache_stats_get(const ffd_ctx* ctx, ffd_cache_stats* out) {
  if (!ctx || !out) return FFD_ERR_INVALID;
  *out = ctx->stats;
  out->table_allocated = ctx->table_allocated ? 1 : 0;
  return FFD_OK;
}

int ffd_cache_tables_read(ffd_ctx* ctx, float* k_out, float* v_out, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!k_out || !v_out) return ctx->fail(FFD_ERR_INVALID, "null buffer");
  if (!ctx->kt) return ctx->fail(FFD_ERR_STATE, "cache not enabled (call ffd_cache_enable)");
  HIPCHECK(hipSetDevice(ctx->device));
  const size_t bytes = ctx->table_floats() * sizeof(float);
  HIPCHECK(hipMemcpyAsync(k_out, ctx->kt, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  HIPCHECK(hipMemcpyAsync(v_out, ctx->vt, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return FFD_OK;
}

// ---------------------------------------------------------------------------
// the sampling loop (sampler.py:156-210)
// ---------------------------------------------------------------------------
// Can this model's sampling step unembed inside the step kernel?  (The loops add their arguments' alignment.)
static bool tail_fusable(const ffd_ctx* ctx) {
  const ffd_model_desc& m = ctx->desc;
  return g_fuse_tail && !ctx->fresca_on && m.kind != FFD_MODEL_MLP && m.kind != FFD_MODEL_MIXTURE &&
         unembed_sde_supported(m.n_channels, m.d_model);
}

// ... and do this call's arguments allow it?  Without FreSca the score is consumed only by the step: unembedding inside
// the step kernel saves one launch and a (B, L, C) round trip per step; FreSca needs the
// whole score (FFT along L).  At C % 4 == 0 the fused kernels read float4 rows: x, the Philox element offset and every
// slab of the injected noise (each aligned like the first) must then sit on 16 bytes.  The ODE tails draw nothing:
// z_inject = nullptr, elem_off = 0; the workspace buffers they also touch are 16-byte aligned.
static bool tail_fuses(const ffd_ctx* ctx, const float* x, const float* z_inject, uint64_t elem_off, size_t slab) {
  if (!tail_fusable(ctx)) return false;
  if (ctx->desc.n_channels % 4 != 0) return true;
  return elem_off % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 &&
         (!z_inject || (reinterpret_cast<uintptr_t>(z_inject) % 16 == 0 && slab % 4 == 0));
}

// FreSca needs two more score-sized buffers.
static int ensure_fresca_work(ffd_ctx* ctx, int B) {
  const ffd_model_desc& m = ctx->desc;
  if (!ctx->fresca_on) return FFD_OK;
  if (int rc = ensure(ctx, ctx->score2, (size_t)B * m.max_len * m.n_channels)) return rc;
  return ensure(ctx, ctx->fwork, (size_t)B * m.n_channels * (m.max_len / 2 + 1) + 4);
}

// All time embeddings of the trajectory in one launch: t is shared by the batch
// (sampler.py:59-60).  The table is kept across batches and only rebuilt (with one
// stream sync) when the timestep grid or the weights changed.
static int ensure_time_table(ffd_ctx* ctx, const float* timesteps, int n_steps, hipStream_t s) {
  const int d = ctx->desc.d_model;
  if ((int)ctx->ts_host.size() == n_steps && memcmp(ctx->ts_host.data(), timesteps, sizeof(float) * n_steps) == 0 &&
      ctx->temb_epoch == ctx->weight_epoch)
    return FFD_OK;
  HIPCHECK(hipStreamSynchronize(s));
  if (int rc = ensure(ctx, ctx->temb_tab, (size_t)n_steps * d)) return rc;
  if (int rc = ensure(ctx, ctx->ts_dev, (size_t)n_steps)) return rc;
  ctx->ts_host.assign(timesteps, timesteps + n_steps);
  HIPCHECK(hipMemcpy(ctx->ts_dev.p, ctx->ts_host.data(), sizeof(float) * n_steps, hipMemcpyHostToDevice));
  if (int rc = time_embed(ctx, ctx->ts_dev.p, 0.f, n_steps, ctx->temb_tab.p, s)) return rc;
  ctx->temb_epoch = ctx->weight_epoch;
  return FFD_OK;
}

// cache.update_crf(crf) with current_step == global step (sampler.py:70-73): where the CRF of the evaluation at global
// step gstep goes (*dst), and a second destination (*copy) when both captures want it; rest = the evaluations of this
// call that still follow
static void crf_capture_targets(const ffd_ctx* ctx, int gstep, int rest, float** dst, float** copy) {
  const ffd_model_desc& m = ctx->desc;
  const ffd_crf_capture_cfg& cc = ctx->crf_cap;
  const size_t crf_n = (size_t)m.num_layers * m.max_len * m.d_model;
  *dst = *copy = nullptr;
  if (cc.ring && gstep % cc.every == 0) *dst = cc.ring + (size_t)((gstep / cc.every) % cc.n_slots) * crf_n;
  if (cc.last && gstep % cc.last_every == 0) {
    const int to_next = cc.last_every - (gstep % cc.last_every);  // is there a later qualifying step in this call?
    if (to_next > rest) {
      if (*dst) *copy = cc.last; else *dst = cc.last;
    }
  }
}

// FreSca on ctx->score at time t (sampler.py:79-93 -> fresca.py:220-268): *score = the buffer that holds the result
static int fresca_score(ffd_ctx* ctx, double t, int B, hipStream_t s, const float** score) {
  const ffd_model_desc& m = ctx->desc;
  const ffd_fresca_cfg& f = ctx->fcfg;
  *score = ctx->score.p;
  double h = (double)f.high_scale;
  if (f.num_steps > 0 && h > 1.0) h = (1.0 - t / (double)f.num_steps) * (h - 1.0) + 1.0;
  if (!((double)f.low_scale == 1.0 && h == 1.0)) {  // fresca.py:137-138 early exit
    HIPCHECK(launch_fresca(ctx->score.p, ctx->score2.p, ctx->fwork.p, B, m.max_len, m.n_channels, f.low_scale, (float)h,
                           f.cutoff_ratio, f.strategy, s));
    *score = ctx->score2.p;
  }
  return FFD_OK;
}

}  // extern "C" (a template follows)

// How every sampling loop starts.  The checks the entries share, in this order: the context, x / timesteps / the range
// [first, first + n_run) within the n_iter iterations the grid offers (steps, intervals or visits), step_size, the
// cache.  Then entry_checks(): the caller's own argument checks, which may rely on the shared ones (a non-zero status
// ends the call).  Only then the device: the workspace, FreSca's buffers, the time table; no multistep history is
// current until the ODE loop says so.  who: the public entry, for the messages.
template <class EntryChecks>
static int loop_begin(ffd_ctx* ctx, const char* who, const float* x, int B, const float* timesteps, int n_steps, int n_iter,
                      int first, int n_run, float step_size, int use_cache, hipStream_t s, EntryChecks entry_checks) {
  int rc = class_check(ctx, who, B, use_cache != 0);  // (first: raised without a device as well)
  if (rc) return rc;
  if ((rc = check_ready(ctx, B))) return rc;
  const int rows = class_stacked(ctx) ? 2 * B : B;  // what one evaluation runs at
  if (rows != B && (rc = check_ready(ctx, rows))) return rc;
  if (!x || !timesteps || n_iter < 1 || first < 0 || n_run < 0 || n_run > n_iter - first)
    return ctx->fail(FFD_ERR_INVALID, "bad argument to %s (n_steps=%d first=%d run=%d of %d)", who, n_steps, first, n_run,
                     n_iter);
  if (!(step_size > 0.f)) return ctx->fail(FFD_ERR_INVALID, "%s: step_size must be > 0 (sde.py:157,238)", who);
  if (use_cache && ctx->desc.kind != FFD_MODEL_TRANSFORMER)
    return ctx->fail(FFD_ERR_UNSUPPORTED, "%s: caching is only defined for the transformer backbone", who);
  if (use_cache && !ctx->cache_enabled) return ctx->fail(FFD_ERR_STATE, "%s: use_cache without ffd_cache_enable", who);
  if ((rc = entry_checks())) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  if ((rc = ensure_workspace(ctx, rows))) return rc;
  if (ctx->class_on) {
    if ((rc = ensure(ctx, ctx->cls_temb, (size_t)rows * ctx->desc.d_model))) return rc;
    if (rows != B && (rc = ensure(ctx, ctx->cls_x, (size_t)rows * ctx->desc.max_len * ctx->desc.n_channels))) return rc;
  }
  if ((rc = ensure_fresca_work(ctx, B))) return rc;
  if ((rc = ensure_time_table(ctx, timesteps, n_steps, s))) return rc;
  ctx->ms_solver = -1;
  ctx->last_parts = 1;  // (run_partitioned says otherwise once both halves are enqueued)
  return FFD_OK;
}

// ---- CU partitions: the batch as two halves that run out of phase ----
// Samples share nothing in the plain Euler-Maruyama loop and in the Euler ODE loop (no cache, no batch statistic, Philox
// counted by the global sample index), so the loop may run as two half-batches, each on a stream confined to its own half
// of every XCD's CUs.  A half is today's launch structure on half the chip; only the memory system couples the two, and
// their load and store bursts no longer fall together.  Ordering is by events alone: a fork on the caller's stream, a
// join per half back onto it.

constexpr int PART_XCDS = 8;  // MI355X; a device whose CU count does not split this way runs single-stream

// The workspace rows of samples [b0, ...) and a CU budget, for the time the calling thread enqueues that half.  The score
// rows start on the next 16-byte boundary (run_partitioned allocates the PART_SCORE_PAD floats that may take): the launchers
// pick a kernel by their pointers' alignment (launch_unembed: the MFMA form or, for a score that is not 16-byte aligned,
// the generic one, which sums in another order), and b0 L C need not be a multiple of 4.
constexpr size_t PART_SCORE_PAD = 3;
struct PartScope {
  ffd_ctx* ctx;
  size_t rows, elems;
  PartScope(ffd_ctx* c, int b0, int budget)
      : ctx(c), rows((size_t)b0 * c->desc.max_len * c->desc.d_model),
        elems(((size_t)b0 * c->desc.max_len * c->desc.n_channels + PART_SCORE_PAD) & ~PART_SCORE_PAD) {
    shift(ctx->h0, rows), shift(ctx->h1, rows), shift(ctx->attn, rows), shift(ctx->score, elems);
    g_cu_budget = budget;
  }
  ~PartScope() {
    g_cu_budget = 0;
    shift(ctx->h0, 0 - rows), shift(ctx->h1, 0 - rows), shift(ctx->attn, 0 - rows), shift(ctx->score, 0 - elems);
  }
  static void shift(Grow<float>& g, size_t n) { g.p += (ptrdiff_t)n, g.cap -= n; }
};

static int ensure_partitions(ffd_ctx* ctx) {
  if (ctx->part_budget) return FFD_OK;
  ctx->part_budget = -1;
  hipDeviceProp_t prop;
  HIPCHECK(hipGetDeviceProperties(&prop, ctx->device));
  const int n = prop.multiProcessorCount, words = (n + 31) / 32;
  std::vector<uint32_t> masks(2 * (size_t)words);
  if (ffd_host_cu_masks(n, PART_XCDS, FFD_CU_LAYOUT_SPREAD, 2, masks.data()) != FFD_OK) return FFD_OK;
  HIPCHECK(hipEventCreateWithFlags(&ctx->part_fork, hipEventDisableTiming));
  for (int p = 0; p < 2; ++p) {
    HIPCHECK(hipExtStreamCreateWithCUMask(&ctx->part_stream[p], (uint32_t)words, masks.data() + (size_t)p * words));
    HIPCHECK(hipEventCreateWithFlags(&ctx->part_join[p], hipEventDisableTiming));
  }
  ctx->part_budget = n / 2;
  return FFD_OK;
}

// CUs per half if this loop call runs partitioned, else 0.  The entry must be one whose loop shares nothing across
// samples (the callers see to that); here: a transformer without cache, FreSca or armed kernel timing, a stream that is
// not being captured, and both halves planned -- for half the CUs -- to the fused attention and an FFN form that keeps no
// partial rows in the shared workspace (ffn_part) and makes no packs on first use.  "partitions" = 1 also wants the
// row-owning FFN with every pass of a half's tiles filling at least 0.9 of its CUs (measured at ECG B = 512 only: 125
// tiles on 128 CUs per half).  Arguments the entry would refuse make the call ineligible, so the single-stream path
// reports them.
// The decision without the call's own arguments (partition_budget adds them; ffd_partition_plan reports it): budget > 0
// to run partitioned; planned: half[] holds the two halves' plans for half the CUs, whatever was decided.
struct PartDecision {
  int budget;
  bool planned;
  LayerPlan half[2];
};
static PartDecision partition_decide(ffd_ctx* ctx, int B, int use_cache) {
  PartDecision d{};
  if (g_partitions == 0 || g_cu_budget > 0 || B < 2) return d;
  if (ctx->desc.kind != FFD_MODEL_TRANSFORMER || !ctx->finalized || !ctx->packs_made() || use_cache || ctx->fresca_on ||
      ctx->class_on || ctx->time_mask)
    return d;
  if (hipSetDevice(ctx->device) != hipSuccess || ensure_partitions(ctx) != FFD_OK || ctx->part_budget <= 0) return d;
  const int budget = ctx->part_budget;
  g_cu_budget = budget;
  bool ok = true;
  int i = 0;
  for (int nb : {(B + 1) / 2, B / 2}) {
    const LayerPlan p = d.half[i++] = plan_of(ctx, nb, CACHE_STD);
    const bool rows = p.ffn == FFN_ROWS_OPROJ || p.ffn == FFN_ROWS;
    ok = ok && p.attn == ATTN_FUSED && p.part_floats == 0 && p.ffn != FFN_SPLIT;
    if (ok && g_partitions == 1) {
      const int last = rows ? cdiv(nb * ctx->desc.max_len, 32 * p.nw) % budget : -1;
      ok = last == 0 || 10 * last >= 9 * budget;
    }
  }
  g_cu_budget = 0;
  d.planned = true;
  d.budget = ok ? budget : 0;
  return d;
}
static int partition_budget(ffd_ctx* ctx, const float* x, int B, const float* timesteps, int n_steps, int n_run,
                            float step_size, int use_cache, hipStream_t s) {
  if (g_partitions == 0 || g_cu_budget > 0 || B < 2 || !x || !timesteps || n_steps < 1 || n_run < 1 || !(step_size > 0.f)) return 0;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return 0;
  return partition_decide(ctx, B, use_cache).budget;
}

// run(b0, nb, first, count, stream): `count` iterations from `first` of the entry's own loop on samples [b0, b0 + nb) with
// their global offsets.  Everything a loop does on first use (workspace growth, the time table and its one
// synchronisation) happens here for the whole batch, on the caller's stream, before the fork; a half then finds it done.
// The halves are enqueued PART_CHUNK iterations at a time, in turn: a hardware queue holds a few thousand launches, and
// the host would otherwise sit in the first half's queue until that half had nearly finished -- the halves then run one
// after the other (10.1 against 5.1 ms per step at ECG B = 512, 1000 steps per call).  A chunk that fails its checks has
// enqueued nothing; the chunks behind it are dropped.
constexpr int PART_CHUNK = 2;
template <class Run>
static int run_partitioned(ffd_ctx* ctx, int budget, int B, const float* timesteps, int n_steps, int first, int n_run,
                           hipStream_t s, Run run) {
  if (int rc = check_ready(ctx, B)) return rc;
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = ensure(ctx, ctx->score, (size_t)B * ctx->desc.max_len * ctx->desc.n_channels + PART_SCORE_PAD)) return rc;
  if (int rc = ensure_workspace(ctx, B)) return rc;
  if (int rc = ensure_time_table(ctx, timesteps, n_steps, s)) return rc;
  HIPCHECK(hipEventRecord(ctx->part_fork, s));
  const int nb0 = (B + 1) / 2;
  int rc = FFD_OK;
  for (int p = 0; p < 2; ++p) HIPCHECK(hipStreamWaitEvent(ctx->part_stream[p], ctx->part_fork, 0));
  for (int j = 0; j < n_run && rc == FFD_OK; j += PART_CHUNK)
    for (int p = 0; p < 2 && rc == FFD_OK; ++p) {
      PartScope scope(ctx, p ? nb0 : 0, budget);
      rc = run(p ? nb0 : 0, p ? B - nb0 : nb0, first + j, n_run - j < PART_CHUNK ? n_run - j : PART_CHUNK, ctx->part_stream[p]);
    }
  for (int p = 0; p < 2; ++p) {
    HIPCHECK(hipEventRecord(ctx->part_join[p], ctx->part_stream[p]));
    HIPCHECK(hipStreamWaitEvent(s, ctx->part_join[p], 0));
  }
  if (rc == FFD_OK) ctx->last_parts = 2;
  return rc;
}

// One plan at nb samples as ffd_partition_plan reports it, for the CUs num_cus() names right now: the names
// ffd_kernel_work gives and the FFN grid the launcher itself computes (RowsArgs::grid_only, ffn_ln_grid)
static void describe_plan(const ffd_ctx* ctx, const LayerPlan& p, int nb, ffd_partition_half* h) {
  const ffd_model_desc& m = ctx->desc;
  const int M = nb * m.max_len;
  h->nb = nb;
  snprintf(h->ffn, sizeof(h->ffn), "%s", kFfnForms[p.ffn].name);
  snprintf(h->attn, sizeof(h->attn), "%s", p.attn == ATTN_FUSED ? "k_qkv_attention" : "k_linear_hm + k_attention_mfma");
  const bool rows = p.ffn == FFN_ROWS_OPROJ || p.ffn == FFN_ROWS, sliced = p.ffn == FFN_ROWS_SLICED_OPROJ || p.ffn == FFN_ROWS_SLICED;
  const bool ln = p.ffn == FFN_LN || p.ffn == FFN_LN_OPROJ;
  h->nw = rows || sliced ? p.nw : 0, h->cps = rows || sliced ? p.cps : 0;
  h->mb = ln ? p.mb : 0, h->persist = p.ffn == FFN_LN ? p.persist : 0;
  h->hpw = p.hpw, h->qg = p.qg, h->kspl = p.kspl;
  h->part_floats = (long long)p.part_floats;
  h->ffn_tiles = h->ffn_grid = 0;
  if (rows || sliced) {
    RowsGrid g{};
    const bool fused = p.ffn == FFN_ROWS_SLICED_OPROJ || p.ffn == FFN_ROWS_OPROJ;
    const RowsArgs a{nullptr, nullptr, &ctx->layers[0], nullptr, M, m.d_model, m.dim_feedforward, p.nw, p.cps, fused,
                     sliced ? p.nslice : 0, nullptr, &g};
    if (launch_ffn_rows(a, nullptr) == hipSuccess) h->ffn_grid = g.grid, h->ffn_tiles = g.ntiles;
  } else if (p.ffn == FFN_LN) {
    h->ffn_grid = ffn_ln_grid(M, p.mb, p.persist, &h->ffn_tiles);
  } else if (p.ffn == FFN_LN_OPROJ) {
    h->ffn_grid = h->ffn_tiles = cdiv(M, 16 * p.mb);  // (launch_oproj_ffn_ln: a workgroup per tile, always)
  }
  h->one_per_tile = h->ffn_grid > 0 && h->ffn_grid == h->ffn_tiles;
}
extern "C" {

int ffd_partition_plan(ffd_ctx* ctx, int B, int entry, ffd_partition_info* info) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!info || B < 1) return ctx->fail(FFD_ERR_INVALID, "bad argument to ffd_partition_plan (B=%d)", B);
  if (entry < FFD_SOLVER_EULER_MARUYAMA || entry > FFD_SOLVER_DPMPP_2M)
    return ctx->fail(FFD_ERR_INVALID, "ffd_partition_plan: entry %d names no sampling loop", entry);
  *info = ffd_partition_info{};
  info->parts = 1;
  info->half[0].nb = (B + 1) / 2, info->half[1].nb = B / 2, info->whole.nb = B;
  // (the loops with state that stays whole-batch never ask: Heun, the multistep solvers, the correctors' entries)
  const bool asks = entry == FFD_SOLVER_EULER_MARUYAMA || entry == FFD_SOLVER_ODE_EULER;
  const PartDecision dec = asks ? partition_decide(ctx, B, 0) : PartDecision{};
  info->cu_budget = ctx->part_budget > 0 ? ctx->part_budget : 0;
  if (dec.budget > 0) info->parts = 2;
  if (dec.planned) {
    g_cu_budget = ctx->part_budget;
    for (int i = 0; i < 2; ++i) describe_plan(ctx, dec.half[i], info->half[i].nb, &info->half[i]);
    g_cu_budget = 0;
    info->halves_planned = 1;
  }
  if (ctx->desc.kind == FFD_MODEL_TRANSFORMER && ctx->finalized && ctx->packs_made() && g_cu_budget == 0) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(FFD_ERR_HIP, "ffd_partition_plan: hipSetDevice failed");
    describe_plan(ctx, plan_of(ctx, B, CACHE_STD), B, &info->whole);
    info->whole_planned = 1;
  }
  return FFD_OK;
}

// One score evaluation of a sampling step, up to where the step's tail takes over: the forward of xin at time-table
// row `row` (time t), the CRF capture, FreSca.  With the cache, a step's first evaluation is `gated`: the gate at global
// step gstep picks its recompute set, its CRF goes where the capture wants it (rest = the gated evaluations of this
// call that still follow), and stats.current_step reads gstep during the forward and the grid index behind it
// (sampler.py:70-74, Q4).  Every later evaluation of the step (Heun's second, the correctors' and the predictor's
// behind them) is a pure hit.  fuse: *hidden = the final hidden rows, which the tail kernel unembeds; otherwise
// *hidden = nullptr and *score = the buffer that holds the (FreSca-scaled) score.
static int loop_evaluate(ffd_ctx* ctx, const float* xin, int row, double t, int B, bool use_cache, bool gated, int gstep,
                         int rest, bool fuse, hipStream_t s, const float** hidden, const float** score) {
  const ffd_model_desc& m = ctx->desc;
  int n_rec = use_cache ? 0 : -1;
  float *crf_dst = nullptr, *crf_copy = nullptr;
  gated = gated && use_cache;
  if (gated) {
    ctx->stats.current_step = gstep;
    n_rec = ffd_host_gate(gstep, m.max_len, ctx->ccfg.K, ctx->ccfg.R);
    if (ctx->crf_cap_on) crf_capture_targets(ctx, gstep, rest, &crf_dst, &crf_copy);
  }
  *hidden = nullptr;
  const float* trow = ctx->temb_tab.p + (size_t)row * m.d_model;
  if (ctx->class_on) {
    // the evaluation's (rows, d) embeddings from the time-table row: the conditional block (g = 0: null labels), and for
    // any g but 0 and 1 the null block behind it, with x copied into both halves of the stacked batch in the same launch.
    // The combine runs on the final hidden rows where the tail is fused, else on the score (the unembedding is affine and
    // the weights sum to 1); the tail and FreSca then see B rows as ever.  (No cache here: class_check refused it.)
    const ffd_class_cfg& c = ctx->ccls;
    const int d = m.d_model;
    const bool stacked = class_stacked(ctx);
    const size_t nx = (size_t)B * m.max_len * m.n_channels;
    HIPCHECK(launch_class_temb(trow, 0, c.table, c.n_classes, c.guidance_scale == 0.f ? nullptr : c.labels, B, d, stacked,
                               ctx->cls_temb.p, xin, stacked ? ctx->cls_x.p : nullptr, nx, s));
    if (int rc = forward_impl(ctx, stacked ? ctx->cls_x.p : xin, ctx->cls_temb.p, d, ctx->score.p, nullptr, stacked ? 2 * B : B,
                              -1, s, fuse ? hidden : nullptr))
      return rc;
    if (stacked) {
      const size_t n = fuse ? (size_t)B * m.max_len * d : nx;
      float* cond = fuse ? const_cast<float*>(*hidden) : ctx->score.p;
      HIPCHECK(launch_cfg_combine(cond, cond + n, c.guidance_scale, n, s));
    }
    *score = ctx->score.p;
    if (ctx->fresca_on) return fresca_score(ctx, t, B, s, score);
    return FFD_OK;
  }
  if (int rc = forward_impl(ctx, xin, trow, 0, ctx->score.p, crf_dst, B, n_rec, s, fuse ? hidden : nullptr)) return rc;
  if (crf_copy)
    HIPCHECK(hipMemcpyAsync(crf_copy, crf_dst, sizeof(float) * (size_t)m.num_layers * m.max_len * m.d_model,
                            hipMemcpyDeviceToDevice, s));
  if (gated) ctx->stats.current_step = row;
  *score = ctx->score.p;
  if (ctx->fresca_on) return fresca_score(ctx, t, B, s, score);
  return FFD_OK;
}

int ffd_sample_batch_ode(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                         int first_step, int n_run, int solver, int use_cache, int global_step0, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  const bool multistep = solver == FFD_SOLVER_ODE_AB2 || solver == FFD_SOLVER_DPMPP_2M;
  const bool heun = solver == FFD_SOLVER_ODE_HEUN;
  const ffd_model_desc& m = ctx->desc;
  const int L = m.max_len, C = m.n_channels, d = m.d_model;
  hipStream_t s = (hipStream_t)stream;
  if (solver == FFD_SOLVER_ODE_EULER)  // (Heun's and the multistep solvers' state buffers stay whole-batch: single-stream)
    if (const int budget = partition_budget(ctx, x, B, timesteps, n_steps, n_run, step_size, use_cache, s))
      return run_partitioned(ctx, budget, B, timesteps, n_steps, first_step, n_run, s,
                             [&](int b0, int nb, int first, int count, hipStream_t ps) {
        return ffd_sample_batch_ode(ctx, x + (size_t)b0 * L * C, nb, timesteps, n_steps, step_size, first, count, solver,
                                    use_cache, global_step0 + (first - first_step), ps);
      });
  std::vector<MultistepParams> ms_coef;
  int rc = loop_begin(ctx, "ffd_sample_batch_ode", x, B, timesteps, n_steps, n_steps > 1 ? n_steps - 1 : 0, first_step,
                      n_run, step_size, use_cache, s, [&]() -> int {
    if (solver != FFD_SOLVER_ODE_EULER && !heun && !multistep)
      return ctx->fail(FFD_ERR_INVALID, "unknown ODE solver %d", solver);
    if (!multistep) return FFD_OK;
    // The multistep solvers: every interval's coefficients.  A trajectory continues (first_step > 0) only on the
    // history the context's previous loop call left for exactly this interval.
    if (first_step > 0 && (ctx->ms_solver != solver || ctx->ms_B != B || ctx->ms_next != first_step))
      return ctx->fail(FFD_ERR_STATE, "first_step=%d continues a multistep trajectory, but the context's previous sampling "
                       "call did not end there with solver %d and B=%d", first_step, solver, B);
    for (int j = 0; j < n_run; ++j) {
      const int i = first_step + j;
      double c[5];
      if (multistep_coef(m.sde, m.sde_a, m.sde_b, solver, i > 0 ? (double)timesteps[i - 1] : 0.0, (double)timesteps[i],
                         (double)timesteps[i + 1], (double)step_size, i > 0, c))
        return ctx->fail(FFD_ERR_INVALID, "interval %d of the grid has no multistep coefficients (times must decrease "
                         "strictly and sigma(t) must be > 0)", i);
      ms_coef.push_back(multistep_params(c));
    }
    return FFD_OK;
  });
  if (rc) return rc;
  if (heun) {  // the predicted state and the predictor's drift
    if ((rc = ensure(ctx, ctx->ode_xp, (size_t)B * L * C))) return rc;
    if ((rc = ensure(ctx, ctx->ode_d1, (size_t)B * L * C))) return rc;
  }
  if (multistep && (rc = ensure(ctx, ctx->ode_hist, (size_t)B * L * C))) return rc;  // (a continued call: already there)
  ctx->tail_solver = solver;  // (multistep: ms_solver is set again once the call's intervals are enqueued)
  float* const xp = ctx->ode_xp.p;
  float* const d1 = ctx->ode_d1.p;
  const bool fuse = tail_fuses(ctx, x, nullptr, 0, 0);
  auto tail = [&](int which, const float* hidden, const float* score, double t) -> hipError_t {
    const SdeParams p = sde_params(m.sde, m.sde_a, m.sde_b, t, step_size);
    if (hidden) return launch_unembed_ode(which, hidden, ctx->model.unembed_w, ctx->model.unembed_b, x, xp, d1, ctx->G_dev, p, B, L, C, d, s);
    return launch_ode_step(which, x, score, xp, d1, ctx->G_dev, p, B, L, C, s);
  };
  for (int j = 0; j < n_run; ++j) {
    const int i = first_step + j;
    const float *hidden, *score;
    const double t = (double)timesteps[i];
    if ((rc = loop_evaluate(ctx, x, i, t, B, use_cache, true, global_step0 + j, n_run - 1 - j, fuse, s, &hidden, &score)))
      return rc;
    if (multistep) {  // history: every interval but a trajectory's first
      if (hidden)
        TIMED(FFD_K_SDE, launch_unembed_multistep(hidden, ctx->model.unembed_w, ctx->model.unembed_b, x, ctx->ode_hist.p,
                                                  ctx->G_dev, ms_coef[j], i > 0, B, L, C, d, s));
      else
        TIMED(FFD_K_SDE, launch_multistep_step(x, score, ctx->ode_hist.p, ctx->G_dev, ms_coef[j], i > 0, B, L, C, s));
      continue;
    }
    TIMED(FFD_K_SDE, tail(heun ? ODE_PREDICT : ODE_EULER, hidden, score, t));
    if (!heun) continue;
    // the corrector's evaluation at (xp, t_{i+1}): with the cache a pure hit
    const double tn = (double)timesteps[i + 1];
    if ((rc = loop_evaluate(ctx, xp, i + 1, tn, B, use_cache, false, 0, 0, fuse, s, &hidden, &score))) return rc;
    TIMED(FFD_K_SDE, tail(ODE_CORRECT, hidden, score, tn));
  }
  if (multistep && first_step + n_run > 0) ctx->ms_solver = solver, ctx->ms_B = B, ctx->ms_next = first_step + n_run;
  return FFD_OK;
}

// The probability-flow ODE walked UPWARD with the divergence of its drift accumulated (include/ffd.h ffd_loglik_batch).
// Interval j runs from timesteps[n - 1 - j] to timesteps[n - 2 - j]; every divergence evaluation is one forward at the
// stacked batch of (1 + 2 k) B rows between a perturbation and a tail launch (ffd_loglik.hip).  The workspace, the
// 32-bit row check and the time table are those of a sampling loop at that many rows.
int ffd_loglik_batch(ffd_ctx* ctx, float* x, double* delta, int B, const float* timesteps, int n_steps, int first_interval,
                     int n_run, int solver, int n_probes, double fd_rel, const float* probe_inject, uint64_t seed,
                     uint64_t sample_offset, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  const ffd_model_desc& m = ctx->desc;
  const int L = m.max_len, C = m.n_channels;
  const bool heun = solver == FFD_SOLVER_ODE_HEUN;
  if (int rc = class_refuse(ctx, "ffd_loglik_batch")) return rc;
  if (B < 1 || n_probes < 1) return ctx->fail(FFD_ERR_INVALID, "ffd_loglik_batch: B=%d, n_probes=%d (both must be >= 1)", B, n_probes);
  if (!loglik_shape_supported(n_probes, B, L, C))
    return ctx->fail(FFD_ERR_UNSUPPORTED, "ffd_loglik_batch: (1 + 2 n_probes) B L C reaches 2^31; shard the batch");
  const int rows = (1 + 2 * n_probes) * B;
  hipStream_t s = (hipStream_t)stream;
  std::vector<float> hs;  // the finite-difference step of every evaluation of the call, in consumption order
  int rc = loop_begin(ctx, "ffd_loglik_batch", x, rows, timesteps, n_steps, n_steps > 1 ? n_steps - 1 : 0, first_interval,
                      n_run, 1.f, 0, s, [&]() -> int {
    if (!delta) return ctx->fail(FFD_ERR_INVALID, "ffd_loglik_batch: null delta");
    if (solver != FFD_SOLVER_ODE_EULER && !heun)
      return ctx->fail(FFD_ERR_INVALID, "ffd_loglik_batch: solver %d is neither FFD_SOLVER_ODE_EULER nor FFD_SOLVER_ODE_HEUN", solver);
    if (!(fd_rel > 0.0 && fd_rel <= 1.7e308)) return ctx->fail(FFD_ERR_INVALID, "ffd_loglik_batch: fd_rel must be > 0 and finite");
    if (ctx->fresca_on)
      return ctx->fail(FFD_ERR_STATE, "ffd_loglik_batch: FreSca is on (call ffd_fresca_disable): a rescaled score is not "
                       "the model's probability-flow ODE");
    if (n_run > 0) {  // the probes' tags of this run stay inside their family (include/ffd.h)
      const int64_t e_max = heun ? 2 * (int64_t)(first_interval + n_run - 1) + 1 : first_interval + n_run - 1;
      if (e_max * n_probes + (n_probes - 1) >= 0x0FFFFFF0ll)
        return ctx->fail(FFD_ERR_INVALID, "ffd_loglik_batch: evaluations x n_probes reaches 0x0FFFFFF0, the end of the "
                         "probes' stream tags");
    }
    const ffd_sde_desc sd{m.sde, 0, m.sde_a, m.sde_b};
    for (int j = 0; j < n_run; ++j) {
      const int lo = n_steps - 1 - (first_interval + j);
      const double t = (double)timesteps[lo], tn = (double)timesteps[lo - 1], dt = tn - t;
      float h0 = 0.f, h1 = 0.f;
      if (!(dt > 0.0) || !((double)(float)dt > 0.0) || ffd_host_loglik_h(&sd, t, fd_rel, &h0) ||
          (heun && ffd_host_loglik_h(&sd, tn, fd_rel, &h1)))
        return ctx->fail(FFD_ERR_INVALID, "ffd_loglik_batch: interval %d of the grid cannot be walked (times must be "
                         "finite, >= 0 and strictly decreasing, with sigma(t) fd_rel > 0 in fp32)", first_interval + j);
      hs.push_back(h0);
      if (heun) hs.push_back(h1);
    }
    return FFD_OK;
  });
  if (rc) return rc;
  const size_t n = (size_t)B * L * C;
  if ((rc = ensure(ctx, ctx->ll_stack, (size_t)rows * L * C))) return rc;
  if (heun) {
    if ((rc = ensure(ctx, ctx->ode_xp, n))) return rc;
    if ((rc = ensure(ctx, ctx->ode_d1, n))) return rc;
    if ((rc = ensure(ctx, ctx->ll_v1, 2 * (size_t)B))) return rc;
  }
  float *const stack = ctx->ll_stack.p, *const xp = ctx->ode_xp.p, *const d1 = ctx->ode_d1.p;
  double* const v1 = reinterpret_cast<double*>(ctx->ll_v1.p);
  const int per = heun ? 2 : 1;  // evaluations per interval
  // evaluation `ev` of the call (ordinal e of the trajectory) at grid row `row`: perturb `at`, forward, tail
  auto evaluate = [&](int stage, const float* at, int ev, int row) -> int {
    const int64_t e = (int64_t)first_interval * per + ev;
    const LoglikProbes pr{probe_inject ? probe_inject + (size_t)ev * n_probes * n : nullptr, seed,
                          sample_offset * (uint64_t)L * C, (uint32_t)(0xF0000000u + (uint32_t)(e * n_probes)), n_probes};
    const double t = (double)timesteps[row];
    const int lo = stage == LL_CORRECT ? row + 1 : row;  // the interval's start row
    const double dt = (double)timesteps[lo - 1] - (double)timesteps[lo];
    TIMED(FFD_K_SDE, launch_loglik_perturb(at, stack, ctx->G_dev, hs[ev], pr, B, L, C, s));
    if (int r = forward_impl(ctx, stack, ctx->temb_tab.p + (size_t)row * m.d_model, 0, ctx->score.p, nullptr, rows, -1, s))
      return r;
    TIMED(FFD_K_SDE, launch_loglik_tail(stage, m.sde, m.sde_a, m.sde_b, t, dt, hs[ev], x, xp, d1, ctx->score.p, ctx->G_dev, pr,
                                        delta, v1, nullptr, B, L, C, s));
    return FFD_OK;
  };
  for (int j = 0; j < n_run; ++j) {
    const int lo = n_steps - 1 - (first_interval + j);
    if (!heun) {
      if ((rc = evaluate(LL_EULER, x, j, lo))) return rc;
      continue;
    }
    if ((rc = evaluate(LL_PREDICT, x, 2 * j, lo))) return rc;
    if ((rc = evaluate(LL_CORRECT, xp, 2 * j + 1, lo - 1))) return rc;
  }
  return FFD_OK;
}

// The visit schedule of resampled conditional sampling (include/ffd.h ffd_host_resample_visit).  Blocks of `jump` grid
// indices (the last may be shorter), each run `resample` times in a row: all blocks before block k are full, so block k
// starts at visit k r j.  *q_out: how many transitions precede this visit's own (the ordinal of the one behind it).
static int resample_visit(int n_steps, int jump, int resample, int visit, int* step_out, int* back_to_out, int* q_out) {
  const int64_t j = jump < n_steps ? jump : n_steps, r = resample, n_blocks = (n_steps + j - 1) / j;
  int64_t k = visit / (r * j);
  if (k > n_blocks - 1) k = n_blocks - 1;
  const int64_t i0 = k * j, len = n_steps - i0 < j ? n_steps - i0 : j, w = visit - k * r * j;
  const int64_t pass = w / len, pos = w % len;
  *step_out = (int)(i0 + pos);
  *back_to_out = pos == len - 1 && pass < r - 1 ? (int)i0 : -1;
  *q_out = (int)(k * (r - 1) + pass);
  return FFD_OK;
}

int ffd_host_resample_visits(int n_steps, int jump, int resample) {
  if (n_steps < 1 || jump < 1 || resample < 1 || (int64_t)n_steps * resample > 0x7FFFFFFFll) return FFD_ERR_INVALID;
  return n_steps * resample;
}

int ffd_host_resample_visit(int n_steps, int jump, int resample, int visit, int* step_out, int* back_to_out) {
  const int n = ffd_host_resample_visits(n_steps, jump, resample);
  if (n < 1 || visit < 0 || visit >= n || !step_out || !back_to_out) return FFD_ERR_INVALID;
  int q;
  return resample_visit(n_steps, jump, resample, visit, step_out, back_to_out, &q);
}

// The stochastic loop behind ffd_sample_batch and its _pc / _cond / _resample forms.  Per reverse step: n_corrector
// Langevin corrector steps (ffd_langevin.hip), then the Euler-Maruyama predictor; with n_corrector == 0 that is plain
// Euler-Maruyama.  cond != nullptr (ffd_sample_batch_cond): one projection onto the observation behind every update, and
// z_inject holds two draws per update (its own, then the projection's).  resample > 1 (ffd_sample_batch_resample):
// first_step and n_run count VISITS of the schedule above, and a visit that ends a pass of its block is followed by one
// forward transition back to the block's first time level (one more slab of z_inject).  The entries check what only
// they take before they call this.
static int sde_loop(ffd_ctx* ctx, const char* who, float* x, int B, const float* timesteps, int n_steps, float step_size,
                    int first_step, int n_run, int n_corrector, float snr, int norm, uint64_t seed, uint64_t sample_offset,
                    const float* z_inject, int use_cache, int global_step0, const ffd_cond_cfg* cond, int jump, int resample,
                    void* stream) {
  const ffd_model_desc& m = ctx->desc;
  const int L = m.max_len, C = m.n_channels, d = m.d_model;
  hipStream_t s = (hipStream_t)stream;
  const int n_visits = n_steps < 1 ? 0 : ffd_host_resample_visits(n_steps, jump, resample);
  int rc = loop_begin(ctx, who, x, B, timesteps, n_steps, n_visits, first_step, n_run, step_size, use_cache, s, [&]() -> int {
    if (!cond && (int64_t)n_steps * n_corrector > 0x7FFFFFF0ll)
      return ctx->fail(FFD_ERR_INVALID, "n_steps * n_corrector exceeds the corrector's Philox tag range");
    if (!cond) return FFD_OK;
    if ((int64_t)n_steps * ((int64_t)n_corrector + 1) > 0x3FFFFFF0ll)
      return ctx->fail(FFD_ERR_INVALID, "n_steps * (n_corrector + 1) exceeds the projection's Philox tag range");
    for (int i = 0; resample > 1 && i < n_steps; ++i)  // a transition runs from a later grid point (or 0) back to an earlier
      if (!(timesteps[i] >= 0.f) || !std::isfinite(timesteps[i]) || (i > 0 && timesteps[i] > timesteps[i - 1]))
        return ctx->fail(FFD_ERR_INVALID, "resampling needs finite, non-increasing timesteps >= 0 (index %d)", i);
    if (!cond->obs || !cond->mask) return ctx->fail(FFD_ERR_INVALID, "conditioning needs obs and mask");
    if (cond->obs_batch != 1 && cond->obs_batch != B)
      return ctx->fail(FFD_ERR_INVALID, "obs_batch must be 1 or B, got %d", cond->obs_batch);
    if (cond->domain != FFD_COND_FREQUENCY && cond->domain != FFD_COND_TIME)
      return ctx->fail(FFD_ERR_INVALID, "unknown conditioning domain %d", cond->domain);
    if (cond->domain == FFD_COND_TIME && cond->std) return ctx->fail(FFD_ERR_INVALID, "std with the time domain");
    if (x == cond->obs || x == cond->mask) return ctx->fail(FFD_ERR_INVALID, "x aliases obs or mask");
    if (cond->domain == FFD_COND_FREQUENCY && !cond_len_supported(L))
      return ctx->fail(FFD_ERR_UNSUPPORTED, "frequency-domain conditioning takes 2 <= L <= 4096");
    return FFD_OK;
  });
  if (rc) return rc;
  if (n_corrector > 0 &&
      (rc = ensure(ctx, ctx->lv_work, (langevin_work_bytes(B, L) + sizeof(float) - 1) / sizeof(float))))
    return rc;
  ctx->tail_solver = n_corrector > 0 ? FFD_SOLVER_PC : FFD_SOLVER_EULER_MARUYAMA;
  const size_t slab = (size_t)B * L * C;
  const size_t zstride = cond ? 2 * slab : slab;  // z_inject per update
  const uint64_t elem_off = sample_offset * (uint64_t)L * C;
  const bool fuse_tail = tail_fuses(ctx, x, z_inject, elem_off, slab);  // (the predictor's; the correctors read the score)
  auto project = [&](double t, int noiseless, const float* z, uint32_t tag) -> hipError_t {
    float mc, sigma;
    cond_coeffs(m.sde, m.sde_a, m.sde_b, t, noiseless, &mc, &sigma);
    if (cond->domain == FFD_COND_TIME)
      return launch_cond_time(x, cond->obs, cond->mask, ctx->G_dev, mc, sigma, noiseless, z, seed, elem_off, tag,
                              cond->obs_batch, B, L, C, s);
    return launch_cond_project(x, cond->obs, cond->mask, cond->std, ctx->G_dev, mc, sigma, noiseless, z, seed, elem_off, tag,
                               cond->obs_batch, B, L, C, s);
  };
  const float* znext = z_inject;  // flat, in execution order: a visit's updates, then its transition's slab
  for (int j = 0; j < n_run; ++j) {
    // visit u of the schedule runs grid index i; without resampling the two are the same.  The Philox tags count visits.
    const int u = first_step + j;
    int i = u, back_to = -1, q = 0;
    if (resample > 1) resample_visit(n_steps, jump, resample, u, &i, &back_to, &q);
    const double t = (double)timesteps[i];
    const float* zj = znext;
    if (znext) znext += (size_t)(n_corrector + 1) * zstride + (back_to >= 0 ? slab : 0);
    for (int k = 0; k <= n_corrector; ++k) {  // k == n_corrector: the predictor
      const bool predictor = k == n_corrector;
      const float *hidden, *score;
      if ((rc = loop_evaluate(ctx, x, i, t, B, use_cache, k == 0, global_step0 + j, n_run - 1 - j, predictor && fuse_tail,
                              s, &hidden, &score)))
        return rc;
      const float* zk = zj ? zj + (size_t)k * zstride : nullptr;
      if (!predictor)
        TIMED(FFD_K_SDE, launch_langevin(x, score, zk, ctx->G_dev, langevin_alpha(m.sde, m.sde_a, m.sde_b, t, step_size),
                                         (double)snr, norm, seed, elem_off,
                                         0x80000000u + (uint32_t)u * (uint32_t)n_corrector + (uint32_t)k, B, L, C, nullptr,
                                         ctx->lv_work.p, s));
      else if (hidden)
        TIMED(FFD_K_SDE, launch_unembed_sde(hidden, ctx->model.unembed_w, ctx->model.unembed_b, x, zk, ctx->G_dev,
                                            sde_params(m.sde, m.sde_a, m.sde_b, t, step_size), seed, elem_off, (uint32_t)u,
                                            B, L, C, d, s));
      else
        TIMED(FFD_K_SDE, launch_sde_step(x, score, zk, ctx->G_dev, sde_params(m.sde, m.sde_a, m.sde_b, t, step_size), seed,
                                         elem_off, (uint32_t)u, B, L, C, s));
      if (cond)
        TIMED(FFD_K_SDE, project(t, 0, zk ? zk + slab : nullptr,
                                 0xC0000000u + (uint32_t)u * (uint32_t)(n_corrector + 1) + (uint32_t)k));
    }
    if (back_to >= 0) {  // the block [back_to, i] runs again: diffuse forward from its end level to its first
      double c[2];
      const double s_end = i + 1 == n_steps ? 0.0 : (double)timesteps[i + 1];
      transition_coef(m.sde, m.sde_a, m.sde_b, s_end, (double)timesteps[back_to], c);  // (0 <= s_end <= t: checked above)
      TIMED(FFD_K_SDE, launch_forward_transition(x, ctx->G_dev, (float)c[0], (float)c[1],
                                                 zj ? zj + (size_t)(n_corrector + 1) * zstride : nullptr, seed, elem_off,
                                                 0xE0000000u + (uint32_t)q, B, L, C, s));
    }
  }
  if (cond && cond->final_replace && n_run > 0 && first_step + n_run == n_visits)
    TIMED(FFD_K_SDE, project((double)timesteps[n_steps - 1], 1, nullptr, 0u));
  return FFD_OK;
}

int ffd_sample_batch(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                     int first_step, int n_run, uint64_t seed, uint64_t sample_offset, const float* z_inject,
                     int use_cache, int global_step0, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  // plain Euler-Maruyama with device draws: a sample's trajectory depends on its global index alone
  if (!z_inject)
    if (const int budget = partition_budget(ctx, x, B, timesteps, n_steps, n_run, step_size, use_cache, (hipStream_t)stream)) {
      const size_t LC = (size_t)ctx->desc.max_len * ctx->desc.n_channels;
      return run_partitioned(ctx, budget, B, timesteps, n_steps, first_step, n_run, (hipStream_t)stream,
                             [&](int b0, int nb, int first, int count, hipStream_t ps) {
        return sde_loop(ctx, "ffd_sample_batch", x + b0 * LC, nb, timesteps, n_steps, step_size, first, count, 0, 0.f, 0, seed,
                        sample_offset + (uint64_t)b0, nullptr, use_cache, global_step0 + (first - first_step), nullptr, 1, 1, ps);
      });
    }
  return sde_loop(ctx, "ffd_sample_batch", x, B, timesteps, n_steps, step_size, first_step, n_run, 0, 0.f, 0, seed,
                  sample_offset, z_inject, use_cache, global_step0, nullptr, 1, 1, stream);
}

// what the entries with correctors check first
static int check_corrector(ffd_ctx* ctx, int n_corrector, float snr, int norm) {
  if (n_corrector < 0) return ctx->fail(FFD_ERR_INVALID, "n_corrector must be >= 0");
  if (!(snr > 0.f)) return ctx->fail(FFD_ERR_INVALID, "snr must be > 0");
  if (norm != FFD_LANGEVIN_NORM_BATCH && norm != FFD_LANGEVIN_NORM_SAMPLE)
    return ctx->fail(FFD_ERR_INVALID, "unknown corrector norm %d", norm);
  return FFD_OK;
}

int ffd_sample_batch_pc(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                        int first_step, int n_run, int n_corrector, float snr, int norm, uint64_t seed,
                        uint64_t sample_offset, const float* z_inject, int use_cache, int global_step0, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (int rc = check_corrector(ctx, n_corrector, snr, norm)) return rc;
  if (n_corrector == 0)
    return ffd_sample_batch(ctx, x, B, timesteps, n_steps, step_size, first_step, n_run, seed, sample_offset, z_inject,
                            use_cache, global_step0, stream);
  return sde_loop(ctx, "ffd_sample_batch_pc", x, B, timesteps, n_steps, step_size, first_step, n_run, n_corrector, snr,
                  norm, seed, sample_offset, z_inject, use_cache, global_step0, nullptr, 1, 1, stream);
}

// Conditional sampling by replacement: the predictor-corrector step with one ffd_cond_project behind every update.
int ffd_sample_batch_cond(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                          int first_step, int n_run, int n_corrector, float snr, int norm, uint64_t seed,
                          uint64_t sample_offset, const float* z_inject, int use_cache, int global_step0,
                          const ffd_cond_cfg* cond, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!cond)
    return ffd_sample_batch_pc(ctx, x, B, timesteps, n_steps, step_size, first_step, n_run, n_corrector, snr, norm, seed,
                               sample_offset, z_inject, use_cache, global_step0, stream);
  if (int rc = check_corrector(ctx, n_corrector, snr, norm)) return rc;
  if (x && z_inject == x) return ctx->fail(FFD_ERR_INVALID, "x aliases z_inject");
  return sde_loop(ctx, "ffd_sample_batch_cond", x, B, timesteps, n_steps, step_size, first_step, n_run, n_corrector, snr,
                  norm, seed, sample_offset, z_inject, use_cache, global_step0, cond, 1, 1, stream);
}

// Resampled conditional sampling ("time travel", RePaint): the conditional loop over the visit schedule above.
int ffd_sample_batch_resample(ffd_ctx* ctx, float* x, int B, const float* timesteps, int n_steps, float step_size,
                              int first_visit, int n_visits, int jump, int resample, int n_corrector, float snr, int norm,
                              uint64_t seed, uint64_t sample_offset, const float* z_inject, const ffd_cond_cfg* cond,
                              void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!cond) return ctx->fail(FFD_ERR_INVALID, "ffd_sample_batch_resample needs an observation (cond)");
  if (jump < 1 || resample < 1) return ctx->fail(FFD_ERR_INVALID, "jump and resample must be >= 1");
  if (int rc = check_corrector(ctx, n_corrector, snr, norm)) return rc;
  if (x && z_inject == x) return ctx->fail(FFD_ERR_INVALID, "x aliases z_inject");
  const int64_t visits = (int64_t)n_steps * resample;  // the projections' tags stay below the transitions' 0xE0000000
  if (visits > 0x1FFFFFF0ll || (visits > 0 && visits * ((int64_t)n_corrector + 1) > 0x1FFFFFF0ll))
    return ctx->fail(FFD_ERR_INVALID, "visits * (n_corrector + 1) reaches the transitions' Philox tags");
  return sde_loop(ctx, "ffd_sample_batch_resample", x, B, timesteps, n_steps, step_size, first_visit, n_visits, n_corrector,
                  snr, norm, seed, sample_offset, z_inject, 0, 0, cond, jump, resample, stream);
}

// Guided conditional sampling (include/ffd.h ffd_sample_batch_guided): per step the score, the seed of the reconstruction
// loss's gradient, the score model's input VJP, the guided score, the stand-alone Euler-Maruyama step and, with
// guide->replace, one projection.  The mixture evaluates both the score and the VJP in closed form; the transformer and
// the MLP take them from `net`, a training object on the same parameters (its forward keeps the activations).
int ffd_sample_batch_guided(ffd_ctx* ctx, ffd_train* net, float* x, int B, const float* timesteps, int n_steps,
                            float step_size, int first_step, int n_run, uint64_t seed, uint64_t sample_offset,
                            const float* z_inject, const ffd_cond_cfg* cond, const ffd_guide_cfg* guide, double* loss_out,
                            void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  const ffd_model_desc& m = ctx->desc;
  const int L = m.max_len, C = m.n_channels;
  const bool mixture = m.kind == FFD_MODEL_MIXTURE;
  hipStream_t s = (hipStream_t)stream;
  std::vector<double> coef;  // (alpha, sigma^2, lambda) of every step of the run
  if (int rc = class_refuse(ctx, "ffd_sample_batch_guided")) return rc;
  int rc = loop_begin(ctx, "ffd_sample_batch_guided", x, B, timesteps, n_steps, n_steps, first_step, n_run, step_size, 0, s,
                      [&]() -> int {
    if (!cond || !guide) return ctx->fail(FFD_ERR_INVALID, "ffd_sample_batch_guided needs an observation (cond) and guide");
    if (m.kind == FFD_MODEL_LSTM)
      return ctx->fail(FFD_ERR_UNSUPPORTED, "ffd_sample_batch_guided: the LSTM has no backward pass");
    if (!mixture) {
      if (!net) return ctx->fail(FFD_ERR_STATE, "ffd_sample_batch_guided: this backbone needs an ffd_train (net) for its VJP");
      const ffd_model_desc& n = train_desc(net);
      if (n.kind != m.kind || n.n_channels != C || n.max_len != L || n.d_model != m.d_model || n.n_head != m.n_head ||
          n.num_layers != m.num_layers || n.dim_feedforward != m.dim_feedforward || n.sde != m.sde || n.sde_a != m.sde_a ||
          n.sde_b != m.sde_b || n.fourier_noise_scaling != m.fourier_noise_scaling || n.eps != m.eps)
        return ctx->fail(FFD_ERR_INVALID, "ffd_sample_batch_guided: net's descriptor differs from the context's");
    }
    if (ctx->fresca_on)
      return ctx->fail(FFD_ERR_STATE, "ffd_sample_batch_guided: FreSca is on (call ffd_fresca_disable): the VJP is the "
                       "unscaled score's");
    if (n_steps > 0x3FFFFFF0) return ctx->fail(FFD_ERR_INVALID, "n_steps exceeds the projection's Philox tag range");
    if (!cond->obs || !cond->mask) return ctx->fail(FFD_ERR_INVALID, "conditioning needs obs and mask");
    if (cond->obs_batch != 1 && cond->obs_batch != B)
      return ctx->fail(FFD_ERR_INVALID, "obs_batch must be 1 or B, got %d", cond->obs_batch);
    if (cond->domain != FFD_COND_FREQUENCY && cond->domain != FFD_COND_TIME)
      return ctx->fail(FFD_ERR_INVALID, "unknown conditioning domain %d", cond->domain);
    if (cond->domain == FFD_COND_TIME && cond->std) return ctx->fail(FFD_ERR_INVALID, "std with the time domain");
    if (x == cond->obs || x == cond->mask || x == z_inject) return ctx->fail(FFD_ERR_INVALID, "x aliases obs, mask or z_inject");
    for (int j = 0; j < n_run; ++j) {
      double c[3];
      if (guide_coef(m.sde, m.sde_a, m.sde_b, (double)timesteps[first_step + j], guide->scale, guide->obs_var, guide->rho, c))
        return ctx->fail(FFD_ERR_INVALID, "ffd_sample_batch_guided: scale, obs_var and rho must be finite and >= 0, the time "
                         "of step %d finite and >= 0 and lambda's denominator there > 0", first_step + j);
      coef.insert(coef.end(), c, c + 3);
    }
    if (cond->domain == FFD_COND_FREQUENCY && !cond_len_supported(L))
      return ctx->fail(FFD_ERR_UNSUPPORTED, "frequency-domain conditioning takes 2 <= L <= 4096");
    return FFD_OK;
  });
  if (rc) return rc;
  const size_t slab = (size_t)B * L * C;
  if ((rc = ensure(ctx, ctx->guide, 3 * ((slab + 3) & ~(size_t)3)))) return rc;
  if (mixture && (rc = ensure(ctx, ctx->mix_work, mixture_vjp_work_floats(B, m.dim_feedforward, L, C)))) return rc;
  ctx->tail_solver = FFD_SOLVER_EULER_MARUYAMA;
  float* const u = ctx->guide.p;
  float* const v = u + ((slab + 3) & ~(size_t)3);
  float* const jtv = v + ((slab + 3) & ~(size_t)3);
  float* const score = ctx->score.p;
  float* const times = ctx->temb_b.p;  // the network's per-sample times (B floats of the (B, d) block)
  const uint64_t elem_off = sample_offset * (uint64_t)L * C;
  auto project = [&](double t, int noiseless, const float* z, uint32_t tag) -> hipError_t {
    float mc, sigma;
    cond_coeffs(m.sde, m.sde_a, m.sde_b, t, noiseless, &mc, &sigma);
    if (cond->domain == FFD_COND_TIME)
      return launch_cond_time(x, cond->obs, cond->mask, ctx->G_dev, mc, sigma, noiseless, z, seed, elem_off, tag,
                              cond->obs_batch, B, L, C, s);
    return launch_cond_project(x, cond->obs, cond->mask, cond->std, ctx->G_dev, mc, sigma, noiseless, z, seed, elem_off, tag,
                               cond->obs_batch, B, L, C, s);
  };
  auto net_call = [&](int r) { return r ? ctx->fail(r, "ffd_sample_batch_guided: net: %s", ffd_train_last_error(net)) : FFD_OK; };
  for (int j = 0; j < n_run; ++j) {
    const int i = first_step + j;
    const double t = (double)timesteps[i];
    const float* tdev = ctx->temb_tab.p + i;  // the mixture's time table is the grid itself (d_model = 1)
    const float* zj = z_inject ? z_inject + (size_t)j * 2 * slab : nullptr;
    if (mixture) {
      if ((rc = forward_impl(ctx, x, tdev, 0, score, nullptr, B, -1, s))) return rc;
    } else {
      HIPCHECK(launch_mixture_times(nullptr, timesteps[i], B, times, s));
      if ((rc = net_call(ffd_train_forward(net, x, times, score, B, stream)))) return rc;
    }
    const GuideArgs ga{x, score, cond->obs, cond->mask, cond->std, ctx->G_dev, u, v, nullptr,
                       loss_out ? loss_out + (size_t)j * B : nullptr, (float)coef[3 * j], (float)coef[3 * j + 1],
                       cond->obs_batch};
    TIMED(FFD_K_SDE, cond->domain == FFD_COND_TIME ? launch_guide_seed_time(ga, B, L, C, s)
                                                   : launch_guide_seed_freq(ga, B, L, C, s));
    if (mixture)
      TIMED(FFD_K_ATTN, launch_mixture_score_vjp(m.sde, m.sde_a, m.sde_b, x, tdev, 0, ctx->mix.means, ctx->mix.logw,
                                                 ctx->mix.var, ctx->G_dev, v, jtv, B, m.dim_feedforward, L, C,
                                                 ctx->mix_work.p, s));
    else if ((rc = net_call(ffd_train_input_vjp(net, v, jtv, B, stream))))
      return rc;
    TIMED(FFD_K_SDE, launch_guide_combine(score, u, jtv, (float)coef[3 * j], (float)coef[3 * j + 2], score, slab, s));
    TIMED(FFD_K_SDE, launch_sde_step(x, score, zj, ctx->G_dev, sde_params(m.sde, m.sde_a, m.sde_b, t, step_size), seed,
                                     elem_off, (uint32_t)i, B, L, C, s));
    if (guide->replace) TIMED(FFD_K_SDE, project(t, 0, zj ? zj + slab : nullptr, 0xC0000000u + (uint32_t)i));
  }
  if (cond->final_replace && n_run > 0 && first_step + n_run == n_steps)
    TIMED(FFD_K_SDE, project((double)timesteps[n_steps - 1], 1, nullptr, 0u));
  return FFD_OK;
}

// ---------------------------------------------------------------------------
// benchmark introspection
// ---------------------------------------------------------------------------
double ffd_flops_per_sample_step(const ffd_ctx* ctx, int cache_hit) {
  if (!ctx) return 0.0;
  const ffd_model_desc& m = ctx->desc;
  const double L = m.max_len, d = m.d_model, C = m.n_channels, NL = m.num_layers, F = m.dim_feedforward;
  if (m.kind == FFD_MODEL_LSTM) return NL * 2.0 * L * (2.0 * 4.0 * d * d) + 4.0 * L * C * d + 2.0 * d * d;
  if (m.kind == FFD_MODEL_MLP) return NL * 4.0 * d * F + 4.0 * L * C * d + 2.0 * d * d;
  // mixture (F carries K): per (component, coordinate) the difference FMA, the product with 1 / c and the sum FMA on
  // the vector pipe (5) and one multiply-add on the matrix cores (2)
  if (m.kind == FFD_MODEL_MIXTURE) return 7.0 * F * L * C;
  double per_layer = 2.0 * L * d * 3.0 * d + 2.0 * L * L * d + 2.0 * L * L * d + 2.0 * L * d * d + 4.0 * L * d * F;
  if (cache_hit) per_layer -= 2.0 * L * d * 2.0 * d;
  return NL * per_layer + 4.0 * L * C * d + 2.0 * d * d;
}

double ffd_ffn_flops_per_launch(const ffd_ctx* ctx, int B) {
  if (!ctx) return 0.0;
  const ffd_model_desc& m = ctx->desc;
  return 4.0 * (double)B * m.max_len * m.d_model * m.dim_feedforward;
}

int ffd_lstm_trace(ffd_ctx* ctx, unsigned long long* host_out, int capacity_units, int* n_units_out) {
  if (!ctx || capacity_units < 1) return FFD_ERR_INVALID;
  HIPCHECK(hipSetDevice(ctx->device));
  if (host_out == nullptr) {  // begin: the next k_lstm_wave launches write their units' records
    if (ctx->lstm_trace) (void)hipFree(ctx->lstm_trace);
    ctx->lstm_trace = nullptr;
    HIPCHECK(hipMalloc(&ctx->lstm_trace, sizeof(unsigned long long) * 4 * (size_t)capacity_units));
    HIPCHECK(hipMemset(ctx->lstm_trace, 0, sizeof(unsigned long long) * 4 * (size_t)capacity_units));
    ctx->lstm_trace_units = capacity_units;
    return FFD_OK;
  }
  if (!ctx->lstm_trace) return ctx->fail(FFD_ERR_STATE, "ffd_lstm_trace: no trace begun");
  HIPCHECK(hipDeviceSynchronize());
  const int n = capacity_units < ctx->lstm_trace_units ? capacity_units : ctx->lstm_trace_units;
  HIPCHECK(hipMemcpy(host_out, ctx->lstm_trace, sizeof(unsigned long long) * 4 * (size_t)n, hipMemcpyDeviceToHost));
  (void)hipFree(ctx->lstm_trace);
  ctx->lstm_trace = nullptr;
  if (n_units_out) *n_units_out = n;
  return FFD_OK;
}

int ffd_kernel_timing_begin(ffd_ctx* ctx, uint32_t class_mask, int max_launches) {
  if (!ctx) return FFD_ERR_INVALID;
  if (max_launches < 1 || max_launches > 100000) return ctx->fail(FFD_ERR_INVALID, "max_launches=%d", max_launches);
  HIPCHECK(hipSetDevice(ctx->device));
  while (ctx->ev.size() < (size_t)2 * max_launches) {
    hipEvent_t e;
    HIPCHECK(hipEventCreate(&e));
    ctx->ev.push_back(e);
  }
  ctx->ev_used = 0;
  ctx->ev_cls.clear();
  ctx->time_mask = class_mask;
  return FFD_OK;
}

int ffd_kernel_timing_end(ffd_ctx* ctx) {
  if (!ctx) return FFD_ERR_INVALID;
  ctx->time_mask = 0;
  HIPCHECK(hipSetDevice(ctx->device));
  double tot[FFD_K_COUNT] = {0};
  for (int c = 0; c < FFD_K_COUNT; ++c) ctx->tm_n[c] = 0;
  const size_t n = ctx->ev_used / 2;
  for (size_t i = 0; i < n; ++i) {
    HIPCHECK(hipEventSynchronize(ctx->ev[2 * i + 1]));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, ctx->ev[2 * i], ctx->ev[2 * i + 1]));
    const int c = ctx->ev_cls[i];
    tot[c] += ms;
    ctx->tm_n[c]++;
  }
  for (int c = 0; c < FFD_K_COUNT; ++c) ctx->tm_ms[c] = ctx->tm_n[c] ? (float)(tot[c] / ctx->tm_n[c]) : 0.f;
  ctx->ev_used = 0;
  ctx->ev_cls.clear();
  return FFD_OK;
}

int ffd_kernel_timing_get(const ffd_ctx* ctx, int kernel_class, float* avg_ms_out, int* launches_out) {
  if (!ctx || kernel_class < 0 || kernel_class >= FFD_K_COUNT || !avg_ms_out || !launches_out) return FFD_ERR_INVALID;
  *avg_ms_out = ctx->tm_ms[kernel_class];
  *launches_out = ctx->tm_n[kernel_class];
  return FFD_OK;
}

const char* ffd_kernel_work(const ffd_ctx* ctx, int kernel_class, int B, int cache_hit, double* flops_out,
                            double* bytes_out) {
  if (!ctx || B < 1) return nullptr;
  const ffd_model_desc& m = ctx->desc;
  const double L = m.max_len, d = m.d_model, C = m.n_channels, F = m.dim_feedforward, M = (double)B * L;
  // (the transformer's forms need the packs ffd_finalize_weights made)
  const bool tr = m.kind == FFD_MODEL_TRANSFORMER && ctx->packs_made(), ls = m.kind == FFD_MODEL_LSTM;
  const LayerPlan p = tr ? plan_of(ctx, B, cache_hit ? CACHE_PURE : CACHE_STD) : LayerPlan{};
  const LstmPlan lp = ls ? plan_lstm(m, B) : LstmPlan{};
  double fl = 0.0, by = 0.0;
  const char* name = nullptr;
  switch (kernel_class) {
    case FFD_K_FFN:  // 4 d F FLOP per row; x in, y out, both weight matrices once (+ the out-projection it absorbs)
      if (tr) {
        const bool op = kFfnForms[p.ffn].oproj;
        name = kFfnForms[p.ffn].name;
        fl = 4.0 * M * d * F + (op ? (p.ffn == FFN_ROWS_SLICED_OPROJ ? p.nslice : 1) * 2.0 * M * d * d : 0.0);
        by = p.ffn == FFN_SPLIT ? 4.0 * (2.0 * M * d) + 6.0 * (2.0 * d * F)
             : op               ? 4.0 * (3.0 * M * d + 2.0 * d * F + d * d)
                                : 4.0 * (2.0 * M * d + 2.0 * d * F);
      }
      break;
    case FFD_K_ATTN:  // in-projection (Q only on a pure-cache step) + QK^T + PV; x in, attention output out
      if (tr) {
        bool any_static = false;  // some layer runs the instance without the per-launch score bound
        for (const LayerWeights& l : ctx->layers) any_static = any_static || (p.attn_static && l.attn_bounded);
        name = p.attn != ATTN_FUSED ? "k_linear_hm + k_attention_mfma"
               : any_static         ? "k_qkv_attention<static bound>"
                                    : "k_qkv_attention";
        fl = M * (2.0 * d * (cache_hit ? d : 3.0 * d) + 4.0 * L * d);
        by = 4.0 * (2.0 * M * d + 3.0 * d * d + (cache_hit ? 2.0 * L * d : 0.0));
        if (p.attn == ATTN_TWO_KERNEL) by += 4.0 * 2.0 * M * (cache_hit ? d : 3.0 * d);  // q / k / v through HBM
      }
      if (m.kind == FFD_MODEL_MIXTURE) {
        // the closed-form mixture score (F carries K): 7 FLOP per (row, component, coordinate); every row tile streams
        // the means once (mostly from L2 / the Infinity Cache), x in, score out, the slices' partials out and in
        const double K = F, D = L * C, tiles = cdiv(B, MIX_ROW_TILE), slices = cdiv((int)F, MIX_SLICE);
        name = "k_mixture_part + k_mixture_merge";
        fl = 7.0 * B * K * D;
        by = 4.0 * (tiles * K * D + 2.0 * B * D + 2.0 * slices * B * (D + 2.0));
      }
      break;
    case FFD_K_OUTPROJ:  // attention output + residual in, LN1 output out
      if (tr && p.oproj_separate) name = "k_linear_res_ln", fl = 2.0 * M * d * d, by = 4.0 * (3.0 * M * d + d * d);
      break;
    case FFD_K_LSTM_REC:
      if (ls && lp.wave) {  // every layer in one launch: x W_ih^T + h W_hh^T; per launch: a sub-batch of Bw samples
        const double Ml = (double)lp.Bw * L;
        name = "k_lstm_wave", fl = m.num_layers * 2.0 * Ml * 8.0 * d * d, by = m.num_layers * 4.0 * (2.0 * Ml * d + 8.0 * d * d);
      }
      else if (ls)  // h W_hh^T for L cell steps; gate pre-activations + residual rows in, rows out
        name = "k_lstm_layer", fl = 2.0 * M * 4.0 * d * d, by = 4.0 * (M * 4.0 * d + 2.0 * M * d + 4.0 * d * d);
      break;
    case FFD_K_LSTM_GATES:
      if (ls && !lp.wave)
        name = "k_linear_rm", fl = 2.0 * M * 4.0 * d * d, by = 4.0 * (M * d + M * 4.0 * d + 4.0 * d * d);
      break;
    case FFD_K_SDE:
      // x, score in; x out (noise generated on chip): 12 B per element; with the unembedding fused
      // into it the score term is replaced by the hidden row: 4 (d + 2 C) B per row
      // The ODE tails of ffd_sample_batch_ode draw nothing.  Euler moves the same bytes; Heun's predictor reads x and
      // writes xp and d1 (3 C floats per row beside the score / hidden row), its corrector reads xp, x, d1 and
      // writes x (4 C): the mean of the two launches is given.
      // The multistep tails (AB2, DPM-Solver++ 2M: one kernel) also read and write the history q: two more (B, L, C)
      // arrays than Euler's, 4 C floats per row beside the score / hidden row (a trajectory's first interval reads no
      // history: 3 C; the figure is the tail's with history).
      // ffd_sample_batch_pc: the predictor's tail is ffd_sample_batch's; per corrector step the class also holds the
      // three (batch norm: four) Langevin launches, which read the score twice and z never: 20 B per element.
      if (ctx->tail_solver == FFD_SOLVER_PC) {
        if (tail_fusable(ctx))
          name = "k_unembed_mfma<sde> + k_lv_rowsq | k_lv_norms | k_lv_update", fl = 2.0 * M * C * d, by = 4.0 * M * (d + 2.0 * C);
        else
          name = "k_sde_step + k_lv_rowsq | k_lv_norms | k_lv_update", by = 12.0 * M * C;
      } else if (ctx->tail_solver == FFD_SOLVER_ODE_HEUN) {
        if (tail_fusable(ctx))
          name = "k_unembed_ode<heun predict | correct>", fl = 2.0 * M * C * d, by = 4.0 * M * (d + 3.5 * C);
        else
          name = "k_ode_step<heun predict | correct>", by = 18.0 * M * C;
      } else if (ctx->tail_solver == FFD_SOLVER_ODE_AB2 || ctx->tail_solver == FFD_SOLVER_DPMPP_2M) {
        if (tail_fusable(ctx))
          name = "k_unembed_multistep", fl = 2.0 * M * C * d, by = 4.0 * M * (d + 4.0 * C);
        else
          name = "k_multistep_step", by = 20.0 * M * C;
      } else if (ctx->tail_solver == FFD_SOLVER_ODE_EULER) {
        if (tail_fusable(ctx))
          name = "k_unembed_ode<euler>", fl = 2.0 * M * C * d, by = 4.0 * M * (d + 2.0 * C);
        else
          name = "k_ode_step<euler>", by = 12.0 * M * C;
      } else if (tail_fusable(ctx))
        name = "k_unembed_mfma<sde>", fl = 2.0 * M * C * d, by = 4.0 * M * (d + 2.0 * C);
      else
        name = "k_sde_step", by = 12.0 * M * C;
      break;
    case FFD_K_EMBED:
      if (m.kind != FFD_MODEL_MLP && m.kind != FFD_MODEL_MIXTURE) name = "k_embed", fl = 2.0 * M * C * d, by = 4.0 * M * (C + d);
      break;
    case FFD_K_UNEMBED:
      if (m.kind != FFD_MODEL_MLP && m.kind != FFD_MODEL_MIXTURE) name = "k_unembed", fl = 2.0 * M * C * d, by = 4.0 * M * (C + d);
      break;
    default: break;
  }
  if (flops_out) *flops_out = fl;
  if (bytes_out) *bytes_out = by;
  return name;
}


}  // extern "C"

// Launches run() back to back: batches of `batch` until warm_seconds have passed (at least one batch), then -- iters
// > 0 -- `iters` launches between a fresh event pair, *ms_out = milliseconds per launch.  The events go on every path.
template <typename Run>
static int time_launches(ffd_ctx* ctx, hipStream_t s, Run run, int batch, double warm_seconds, int iters, float* ms_out) {
  struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } ev;
  HIPCHECK(hipEventCreate(&ev.e0));
  HIPCHECK(hipEventCreate(&ev.e1));
  HIPCHECK(hipEventRecord(ev.e0, s));
  float ms = 0.f;
  do {
    for (int i = 0; i < batch; ++i) HIPCHECK(run());
    HIPCHECK(hipEventRecord(ev.e1, s));
    HIPCHECK(hipEventSynchronize(ev.e1));
    HIPCHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  } while (ms * 1e-3 < warm_seconds);
  if (iters < 1) return FFD_OK;
  HIPCHECK(hipEventRecord(ev.e0, s));
  for (int i = 0; i < iters; ++i) HIPCHECK(run());
  HIPCHECK(hipEventRecord(ev.e1, s));
  HIPCHECK(hipEventSynchronize(ev.e1));
  HIPCHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *ms_out = ms / iters;
  return FFD_OK;
}

extern "C" {

struct StampBuf {  // a probe's stamp records on the device, freed on every path
  unsigned long long* p = nullptr;
  ~StampBuf() { (void)hipFree(p); }
};

// Common set-up of the FFN probes: layer 0's planned FFD_K_FFN launch(es) at batch B on random rows (attention output
// in ctx->attn, residual rows in h1, x1 in h0 for the forms behind k_linear_res_ln)
static int ffn_probe_setup(ffd_ctx* ctx, int B, hipStream_t s, LayerPlan* plan) {
  if (int rc = check_ready(ctx, B)) return rc;
  if (ctx->desc.kind != FFD_MODEL_TRANSFORMER) return ctx->fail(FFD_ERR_UNSUPPORTED, "no FFN in this backbone");
  HIPCHECK(hipSetDevice(ctx->device));
  if (int rc = ensure_workspace(ctx, B)) return rc;
  *plan = plan_of(ctx, B, CACHE_STD);
  if (plan->ffn == FFN_SPLIT && ctx->layers[0].w1s == nullptr)
    return ctx->fail(FFD_ERR_STATE, "ffn_split: run one forward first (the packs are made on first use)");
  if (int rc = ensure(ctx, ctx->ffn_part, plan->part_floats)) return rc;
  const size_t n = (size_t)B * ctx->desc.max_len * ctx->desc.d_model;
  hipLaunchKernelGGL(k_fill_hash, dim3(1024), dim3(256), 0, s, ctx->h1.p, n, 0x9E3779B9u);
  hipLaunchKernelGGL(k_fill_hash, dim3(1024), dim3(256), 0, s, ctx->attn.p, n, 0x85EBCA6Bu);
  hipLaunchKernelGGL(k_fill_hash, dim3(1024), dim3(256), 0, s, ctx->h0.p, n, 0xC2B2AE35u);
  HIPCHECK(hipGetLastError());
  return FFD_OK;
}

int ffd_bench_ffn(ffd_ctx* ctx, int B, int iters, float* ms_out, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (iters < 1 || !ms_out) return ctx->fail(FFD_ERR_INVALID, "bad argument to ffd_bench_ffn");
  hipStream_t s = (hipStream_t)stream;
  LayerPlan p;
  if (int rc = ffn_probe_setup(ctx, B, s, &p)) return rc;
  const int M = B * ctx->desc.max_len;
  auto run = [&]() { return run_ffn(ctx, p, ctx->layers[0], ctx->attn.p, ctx->h1.p, ctx->h0.p, M, s); };
  return time_launches(ctx, s, run, 3, 0.0, iters, ms_out);
}

int ffd_probe_ffn_clock(ffd_ctx* ctx, int B, double warm_seconds, double* ghz_out, double* loop_us_out,
                        unsigned long long* raw_out, int raw_capacity, int* nwg_out, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  if (!ghz_out || !(warm_seconds >= 0.0) || warm_seconds > 30.0) return ctx->fail(FFD_ERR_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  LayerPlan p;
  if (int rc = ffn_probe_setup(ctx, B, s, &p)) return rc;
  const int M = B * ctx->desc.max_len;
  const int nwg = cdiv(M, 16);  // upper bound of every form's grid (16-row tiles at the smallest)
  StampBuf stamps;
  HIPCHECK(hipMalloc((void**)&stamps.p, sizeof(unsigned long long) * 8 * nwg));
  HIPCHECK(hipMemsetAsync(stamps.p, 0, sizeof(unsigned long long) * 8 * nwg, s));
  auto launch = [&](unsigned long long* st) { return run_ffn(ctx, p, ctx->layers[0], ctx->attn.p, ctx->h1.p, ctx->h0.p, M, s, st); };
  // back-to-back launches for warm_seconds (the clock the chip settles at under this load), then the stamped one
  float unused;
  if (int rc = time_launches(ctx, s, [&]() { return launch(nullptr); }, 50, warm_seconds, 0, &unused)) return rc;
  if (launch(stamps.p) != hipSuccess)
    return ctx->fail(FFD_ERR_UNSUPPORTED, "no stamped twin of the planned FFN form (%s)", kFfnForms[p.ffn].name);
  std::vector<unsigned long long> h(8 * (size_t)nwg);
  HIPCHECK(hipMemcpyAsync(h.data(), stamps.p, sizeof(unsigned long long) * 8 * nwg, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  std::vector<double> ghz, us;
  int used = 0;
  for (int i = 0; i < nwg; ++i)
    if (h[8 * i + 1] > 0) {
      ghz.push_back((double)h[8 * i] / (double)h[8 * i + 1] * 0.1);  // shader cycles per 10 ns tick
      us.push_back((double)h[8 * i + 1] * 0.01);
      if (raw_out && used < raw_capacity) memcpy(raw_out + 8 * (size_t)used, &h[8 * i], sizeof(unsigned long long) * 8);
      ++used;
    }
  if (nwg_out) *nwg_out = used;
  if (ghz.empty()) return ctx->fail(FFD_ERR_STATE, "no stamps were written");
  std::sort(ghz.begin(), ghz.end());
  std::sort(us.begin(), us.end());
  *ghz_out = ghz[ghz.size() / 2];
  if (loop_us_out) *loop_us_out = us[us.size() / 2];
  return FFD_OK;
}

int ffd_async_status(ffd_ctx* ctx) {
  if (!ctx) return FFD_ERR_INVALID;
  return check_async(ctx);
}

int ffd_probe_attn(ffd_ctx* ctx, int B, int n_recompute, double warm_seconds, int iters, float* ms_out,
                   unsigned long long* raw_out, int raw_capacity, int* nrec_out, void* stream) {
  if (!ctx) return FFD_ERR_INVALID;
  int rc = check_ready(ctx, B);
  if (rc) return rc;
  const ffd_model_desc& m = ctx->desc;
  if (m.kind != FFD_MODEL_TRANSFORMER) return ctx->fail(FFD_ERR_UNSUPPORTED, "no attention in this backbone");
  if (!ms_out || iters < 1 || !(warm_seconds >= 0.0) || warm_seconds > 30.0) return ctx->fail(FFD_ERR_INVALID, "bad argument");
  const int L = m.max_len, d = m.d_model, H = m.n_head;
  if (n_recompute > L) return ctx->fail(FFD_ERR_INVALID, "n_recompute=%d outside [-1,%d]", n_recompute, L);
  const CacheMode mode = cache_mode(n_recompute, L);  // (FULL reads no tables: the plain layer's launch)
  const CacheUse cu = cache_use(mode, n_recompute, L);
  if (cu.tables && !(ctx->cache_enabled && ctx->table_allocated))
    return ctx->fail(FFD_ERR_STATE, "cached modes need ffd_cache_enable and one full step (the tables)");
  HIPCHECK(hipSetDevice(ctx->device));
  if ((rc = ensure_workspace(ctx, B))) return rc;
  const LayerPlan p = plan_of(ctx, B, mode);
  if (p.attn == ATTN_TWO_KERNEL)
    if ((rc = ensure(ctx, ctx->qkv, (size_t)B * L * 3 * d))) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_fill_hash, dim3(1024), dim3(256), 0, s, ctx->h1.p, (size_t)B * L * d, 0x9E3779B9u);  // random rows
  HIPCHECK(hipGetLastError());
  // (MIXED: the recomputed rows of batch element 0 are NOT written back -- the probe leaves the tables as they are)
  // (layer 1 where there is one: layer 0 never takes the static-bound instance the other layers may run)
  auto launch = [&](unsigned long long* st) {
    return run_attention(ctx, p, ctx->layers[m.num_layers > 1 ? 1 : 0], ctx->h1.p, cu.tables ? ctx->kt : nullptr, cu.tables ? ctx->vt : nullptr,
                         nullptr, nullptr, B, cu.n_own, s, st);
  };
  if ((rc = time_launches(ctx, s, [&]() { return launch(nullptr); }, 20, warm_seconds, iters, ms_out))) return rc;
  if (nrec_out) *nrec_out = 0;
  if (raw_out && raw_capacity > 0) {
    const size_t nwave = (size_t)B * H * 4;  // upper bound: at most 4 waves per (sample, head) workgroup / head pair
    StampBuf stamps;
    HIPCHECK(hipMalloc((void**)&stamps.p, sizeof(unsigned long long) * 16 * nwave));
    HIPCHECK(hipMemsetAsync(stamps.p, 0, sizeof(unsigned long long) * 16 * nwave, s));
    if (launch(stamps.p) != hipSuccess)
      return ctx->fail(FFD_ERR_UNSUPPORTED, "no stamped twin of the planned attention form (%s, %d head(s) per workgroup, "
                       "pack mode %d, %d key pieces) for this shape", p.attn == ATTN_FUSED ? "k_qkv_attention" : "two-kernel",
                       p.hpw, p.q_only, p.kspl);
    std::vector<unsigned long long> h(16 * nwave);
    HIPCHECK(hipMemcpyAsync(h.data(), stamps.p, sizeof(unsigned long long) * 16 * nwave, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    int used = 0;
    for (size_t i = 0; i < nwave && used < raw_capacity; ++i)
      if (h[16 * i + 1] != 0) memcpy(raw_out + 16 * (size_t)used++, &h[16 * i], sizeof(unsigned long long) * 16);
    if (nrec_out) *nrec_out = used;
  }
  return FFD_OK;
}

}  // extern "C"
