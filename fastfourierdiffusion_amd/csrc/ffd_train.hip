// Training on the device: the backward pass of the dense layers, LayerNorm and attention, the loss gradient, the gradient
// norm and AdamW, and the training object that runs them for the transformer and the MLP score networks (ScoreModule,
// MLPScoreModule; score_models.py:79-119, 290-324, 363-440).
//
//   k_dense_dgrad     dX[M,K] = mask(dY[M,N] . W[N,K]) + R      64 x 64 output tile per workgroup, N walked 32 at a time
//   k_dense_wgrad     dW[N,K] = dY^T . X, db[N] = column sums   64 x 64 tile per workgroup and chunk of M (wgrad_plan)
//   k_wgrad_reduce    the chunks' partial tiles added in chunk order (fp64)
//   k_train_perturb   the perturbation of ffd_sm_perturb with an optional row index; one workgroup per sample
//   k_sm_loss_grad    the per-sample losses of k_sm_loss and d loss / d score
//   k_time_features   [sin(2 pi t W), cos(2 pi t W)][:d], kept for the time encoder's weight gradient
//   k_sqnorm_seg / k_sqnorm_final   the squared gradient norm over every bound tensor, two fixed-order fp64 trees
//   k_adamw(_seg)     torch.optim.AdamW's update with the clip coefficient read from the device
//
// Both GEMMs stage their operands through LDS (a tile is read from HBM once per workgroup) and run on
// v_mfma_f32_16x16x4_f32: a wave owns 16 x 64 of the output tile, four independent accumulators.  The next step's
// operands are loaded into registers under the MFMAs of the current one.  Rows, columns and reduction indices beyond
// the edges read as zero, so any M, N, K is taken (no float4 path: K % 4 != 0 needs no second instance).
// Nothing uses atomics; every result is bit-identical from run to run.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "ffd_internal.h"

namespace ffd {

constexpr int TG_TILE = 64;       // output rows and columns per workgroup
constexpr int TG_STEP = 32;       // reduction indices per LDS stage
constexpr int TG_LD = 80;         // row stride of a [32][64] stage: 80 % 32 == 16, so k-rows q, q + 1 of a half-wave read disjoint banks
constexpr int TG_LDA = 34;        // row stride of the [64][32] stage of k_dense_dgrad (lds_stride(32))
constexpr int WGRAD_ROWS = 1024;  // rows of M per chunk (at most), WGRAD_MAX_CHUNKS chunks
constexpr int WGRAD_MAX_CHUNKS = 64;
constexpr int WGRAD_MIN_ROWS = 64;   // ... and no finer than this, however few output tiles there are
constexpr int WGRAD_FILL = 256;      // workgroups the finer cut aims at (a constant, not the device's CU count: the plan,
                                     // and with it the order of every sum, depends on the shape alone)

// ---- dgrad ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_dgrad(const float* __restrict__ dY, const float* __restrict__ W,
                                                     const float* __restrict__ act, const float* __restrict__ R,
                                                     float* __restrict__ dX, int M, int N, int K) {
  __shared__ float sA[TG_TILE * TG_LDA];  // dY[m0 + mm][n0 + nn]
  __shared__ float sB[TG_STEP * TG_LD];   // W[n0 + nn][k0 + kk]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * TG_TILE, k0 = blockIdx.y * TG_TILE;  // M, the long dimension, on grid.x
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ra[8], rb[8];
  auto gload = [&](int n0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i;
      const int am = m0 + (e >> 5), an = n0 + (e & 31);
      ra[i] = (am < M && an < N) ? dY[(size_t)am * N + an] : 0.f;
      const int bn = n0 + (e >> 6), bk = k0 + (e & 63);
      rb[i] = (bn < N && bk < K) ? W[(size_t)bn * K + bk] : 0.f;
    }
  };
  gload(0);
  for (int n0 = 0; n0 < N; n0 += TG_STEP) {
    __syncthreads();  // the previous stage has been read
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i;
      sA[(e >> 5) * TG_LDA + (e & 31)] = ra[i];
      sB[(e >> 6) * TG_LD + (e & 63)] = rb[i];
    }
    __syncthreads();
    if (n0 + TG_STEP < N) gload(n0 + TG_STEP);
#pragma unroll
    for (int s = 0; s < TG_STEP / 4; ++s) {
      const float a = sA[(16 * wave + r) * TG_LDA + 4 * s + q];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma16(a, sB[(4 * s + q) * TG_LD + 16 * t + r], acc[t]);
    }
  }
  // D: lane holds rows 4q + i (i = 0..3) of column r of each 16 x 16 tile
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + 16 * t + r;
    if (k >= K) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + 16 * wave + 4 * q + i;
      if (m >= M) continue;
      const size_t o = (size_t)m * K + k;
      float v = acc[t][i];
      if (act && !(act[o] > 0.f)) v = 0.f;  // the saved post-ReLU activation is positive where the pre-activation was
      if (R) v += R[o];
      dX[o] = v;
    }
  }
}

hipError_t launch_dense_dgrad(const float* dY, const float* W, const float* act, const float* R, float* dX, int M, int N,
                              int K, hipStream_t s) {
  hipLaunchKernelGGL(k_dense_dgrad, dim3(cdiv(M, TG_TILE), cdiv(K, TG_TILE)), dim3(256), 0, s, dY, W, act, R, dX, M, N, K);
  return hipGetLastError();
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------
// M is cut into nchunks chunks of `rows` rows (a multiple of 32).  A function of the shape alone: chunks of at most
// WGRAD_ROWS rows; where the output has few 64 x 64 tiles, finer, until tiles x chunks reaches WGRAD_FILL workgroups or a
// chunk is down to WGRAD_MIN_ROWS rows (a 512-row batch against a 187 x 72 weight: 6 tiles x 8 chunks of 64 rows).
struct WgradPlan {
  int rows, nchunks;
};
static WgradPlan wgrad_plan(int M, int N, int K) {
  const long tiles = (long)cdiv(N, TG_TILE) * cdiv(K, TG_TILE);
  long n = cdiv(M, WGRAD_ROWS);
  const long fill = (WGRAD_FILL + tiles - 1) / tiles, finest = cdiv(M, WGRAD_MIN_ROWS);
  n = std::max(n, std::min(fill, finest));
  n = std::min<long>(n, WGRAD_MAX_CHUNKS);
  const int rows = cdiv(cdiv(M, (int)n), TG_STEP) * TG_STEP;
  return {rows, cdiv(M, rows)};
}
// one chunk: written straight to dW / db; else [nchunks][N] doubles (bias) then [nchunks][N][K] floats
static size_t wgrad_work_bytes(int M, int N, int K) {
  const WgradPlan p = wgrad_plan(M, N, K);
  if (p.nchunks == 1) return 0;
  return (size_t)p.nchunks * N * sizeof(double) + (size_t)p.nchunks * N * K * sizeof(float);
}

__global__ __launch_bounds__(256) void k_dense_wgrad(const float* __restrict__ dY, const float* __restrict__ X,
                                                     float* __restrict__ dW, float* __restrict__ db,
                                                     float* __restrict__ partW, double* __restrict__ partb, int M, int N,
                                                     int K, int rows) {
  __shared__ float sA[TG_STEP * TG_LD];  // dY[mb + mm][n0 + c]
  __shared__ float sB[TG_STEP * TG_LD];  // X[mb + mm][k0 + c]
  __shared__ double sred[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int k0 = blockIdx.x * TG_TILE, n0 = blockIdx.y * TG_TILE, chunk = blockIdx.z;
  const int mbeg = chunk * rows, mend = min(M, mbeg + rows);
  const bool bias = blockIdx.x == 0 && (db || partb);
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  double bsum = 0.0;
  float ra[8], rb[8];
  auto gload = [&](int mb) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i;
      const int m = mb + (e >> 6), c = e & 63;
      ra[i] = (m < mend && n0 + c < N) ? dY[(size_t)m * N + n0 + c] : 0.f;
      rb[i] = (m < mend && k0 + c < K) ? X[(size_t)m * K + k0 + c] : 0.f;
    }
  };
  gload(mbeg);
  for (int mb = mbeg; mb < mend; mb += TG_STEP) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i;
      sA[(e >> 6) * TG_LD + (e & 63)] = ra[i];
      sB[(e >> 6) * TG_LD + (e & 63)] = rb[i];
    }
    __syncthreads();
    if (mb + TG_STEP < mend) gload(mb + TG_STEP);
#pragma unroll
    for (int s = 0; s < TG_STEP / 4; ++s) {
      const float a = sA[(4 * s + q) * TG_LD + 16 * wave + r];  // A[i = n][k = m]
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma16(a, sB[(4 * s + q) * TG_LD + 16 * t + r], acc[t]);
    }
    if (bias) {  // thread: column tid & 63, rows 8 (tid >> 6) .. + 7 of the stage, in order
#pragma unroll
      for (int j = 0; j < 8; ++j) bsum += (double)sA[(8 * wave + j) * TG_LD + lane];
    }
  }
  if (bias) {
    sred[tid] = bsum;
    __syncthreads();
    if (tid < 64 && n0 + tid < N) {
      const double tot = ((sred[tid] + sred[tid + 64]) + sred[tid + 128]) + sred[tid + 192];
      if (partb) partb[(size_t)chunk * N + n0 + tid] = tot;
      else db[n0 + tid] = (float)tot;
    }
  }
  float* out = partW ? partW + (size_t)chunk * N * K : dW;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + 16 * t + r;
    if (k >= K) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + 16 * wave + 4 * q + i;
      if (n < N) out[(size_t)n * K + k] = acc[t][i];
    }
  }
}

__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ partW, const double* __restrict__ partb,
                                                      float* __restrict__ dW, float* __restrict__ db, size_t NK, int N,
                                                      int nchunks) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < NK) {
    double a = 0.0;
    for (int c = 0; c < nchunks; ++c) a += (double)partW[(size_t)c * NK + i];
    dW[i] = (float)a;
  }
  if (db && i < (size_t)N) {
    double a = 0.0;
    for (int c = 0; c < nchunks; ++c) a += partb[(size_t)c * N + i];
    db[i] = (float)a;
  }
}

// work: wgrad_work_bytes(M, N, K) bytes, 8-byte aligned (unused with one chunk)
hipError_t launch_dense_wgrad(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, void* work,
                              hipStream_t s) {
  const WgradPlan p = wgrad_plan(M, N, K);
  const dim3 grid(cdiv(K, TG_TILE), cdiv(N, TG_TILE), p.nchunks);
  if (p.nchunks == 1) {
    hipLaunchKernelGGL(k_dense_wgrad, grid, dim3(256), 0, s, dY, X, dW, db, (float*)nullptr, (double*)nullptr, M, N, K,
                       p.rows);
    return hipGetLastError();
  }
  double* partb = (double*)work;
  float* partW = (float*)(partb + (size_t)p.nchunks * N);
  hipLaunchKernelGGL(k_dense_wgrad, grid, dim3(256), 0, s, dY, X, dW, db, partW, db ? partb : (double*)nullptr, M, N, K,
                     p.rows);
  if (hipError_t e = hipGetLastError()) return e;
  const size_t NK = (size_t)N * K;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, s, partW, partb, dW, db, NK, N,
                     p.nchunks);
  return hipGetLastError();
}

// ---- perturbation with a row index, loss gradient ---------------------------------------------------------------------
// Sample b of the call is row `row` = index ? index[b] : b of x0 and draws as global sample sample_offset + row: the
// values ffd_sm_perturb gives that row, whatever batch it is in.  t, mc, sigma are in batch order (B).
__global__ __launch_bounds__(256) void k_train_perturb(const float* __restrict__ x0, float* __restrict__ xn,
                                                       const float* __restrict__ t, const float* __restrict__ mc,
                                                       const float* __restrict__ sigma, const float* __restrict__ G,
                                                       const float* __restrict__ z, uint64_t seed, uint64_t sample_offset,
                                                       const int64_t* __restrict__ index, float* __restrict__ t_b,
                                                       float* __restrict__ sigma_b, unsigned L, unsigned C) {
  const unsigned b = blockIdx.x, n = L * C;
  const uint64_t row = index ? (uint64_t)index[b] : (uint64_t)b;
  const float m = mc[b], sg = sigma[b];
  if (threadIdx.x == 0) t_b[b] = t[b], sigma_b[b] = sg;
  const uint64_t g0 = (sample_offset + row) * (uint64_t)n, g1 = g0 + n;
  const float* xr = x0 + (size_t)row * n;
  const size_t base = (size_t)b * n;
  for (uint64_t qd = (g0 >> 2) + threadIdx.x; qd <= ((g1 - 1) >> 2); qd += 256) {
    float zz[4];
    if (!z) normal4(qd, seed, SM_TAG_NOISE, zz);
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
      const uint64_t g = (qd << 2) + j;
      if (g < g0 || g >= g1) continue;
      const unsigned e = (unsigned)(g - g0);
      const float zv = z ? z[base + e] : zz[j];
      xn[base + e] = __fadd_rn(__fmul_rn(m, xr[e]), __fmul_rn(__fmul_rn(sg, G[e / C]), zv));  // as ffd_sm_perturb
    }
  }
}

// k_sm_loss (reduce_mean) with the gradient: the same terms added in the same order, so out[b] has ffd_sm_loss's bits;
// dscore = 2 w_b r / (L C B), or 2 std^2 r / (L C B) with likelihood weighting, formed in fp64 and rounded once.
template <bool LW>
__global__ __launch_bounds__(256) void k_sm_loss_grad(const float* __restrict__ score, const float* __restrict__ sigma,
                                                      const float* __restrict__ G, const float* __restrict__ z,
                                                      uint64_t seed, uint64_t sample_offset,
                                                      const int64_t* __restrict__ index, double* __restrict__ out,
                                                      float* __restrict__ dscore, unsigned L, unsigned C, unsigned B) {
  __shared__ double red[256];
  const unsigned b = blockIdx.x, n = L * C;
  const float sg = sigma[b];
  const uint64_t gs = sample_offset + (index ? (uint64_t)index[b] : (uint64_t)b);
  const uint64_t g0 = gs * (uint64_t)n, g1 = g0 + n;
  const size_t base = (size_t)b * n;
  const double inv_nB = 1.0 / ((double)n * (double)B);
  double wsum = 1.0;
  if (!LW) {  // weighting_factor = 1 / sum_l (1 / std^2) (losses.py:96)
    double ws = 0.0;
    for (unsigned l = threadIdx.x; l < L; l += 256) {
      const double sd = (double)__fmul_rn(sg, G[l]);
      ws += 1.0 / (sd * sd);
    }
    wsum = block_sum(ws, red);
  }
  const double coef = 2.0 * inv_nB / wsum;
  double acc = 0.0;
  for (uint64_t qd = (g0 >> 2) + threadIdx.x; qd <= ((g1 - 1) >> 2); qd += 256) {
    float zz[4];
    if (!z) normal4(qd, seed, SM_TAG_NOISE, zz);
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
      const uint64_t g = (qd << 2) + j;
      if (g < g0 || g >= g1) continue;
      const unsigned e = (unsigned)(g - g0);
      const float zv = z ? z[base + e] : zz[j];
      const float sd = __fmul_rn(sg, G[e / C]);
      const float r = __fadd_rn(score[base + e], __fmul_rn(__fdiv_rn(1.0f, sd), zv));
      const float qq = LW ? __fmul_rn(sd, r) : r;
      acc += (double)__fmul_rn(qq, qq);
      dscore[base + e] = LW ? (float)(2.0 * inv_nB * ((double)sd * (double)sd) * (double)r) : (float)(coef * (double)r);
    }
  }
  double total = block_sum(acc, red);
  if (!LW) total /= wsum;
  if (threadIdx.x == 0) out[b] = total / (double)n;
}

hipError_t launch_sm_loss_grad(const float* score, const float* sigma, const float* G, const float* z, uint64_t seed,
                               uint64_t sample_offset, const int64_t* index, int likelihood_weighting, double* out,
                               float* dscore, int B, int L, int C, hipStream_t s) {
  if (likelihood_weighting)
    hipLaunchKernelGGL(k_sm_loss_grad<true>, dim3((unsigned)B), dim3(256), 0, s, score, sigma, G, z, seed, sample_offset,
                       index, out, dscore, (unsigned)L, (unsigned)C, (unsigned)B);
  else
    hipLaunchKernelGGL(k_sm_loss_grad<false>, dim3((unsigned)B), dim3(256), 0, s, score, sigma, G, z, seed, sample_offset,
                       index, out, dscore, (unsigned)L, (unsigned)C, (unsigned)B);
  return hipGetLastError();
}

// emb[b][j] = sin / cos(((t W) 2) pi), the features k_time_embed forms (transformer.py:77-91)
__global__ __launch_bounds__(256) void k_time_features(const float* __restrict__ ts, const float* __restrict__ W,
                                                       float* __restrict__ emb, int B, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D) return;
  const int b = i / D, j = i - b * D, half = (D + 1) / 2;
  const float w = W[j < half ? j : j - half];
  const float proj = __fmul_rn(__fmul_rn(__fmul_rn(ts[b], w), 2.0f), 3.14159265358979323846f);
  emb[i] = j < half ? sinf(proj) : cosf(proj);
}

// ---- gradient norm and AdamW ------------------------------------------------------------------------------------------
constexpr unsigned TRAIN_SEG = 4096;  // elements per segment of the tables below
struct TrainSeg {
  float* p;
  const float* g;
  float *m, *v;
  unsigned n, pad;
};

__global__ __launch_bounds__(256) void k_sqnorm_seg(const TrainSeg* __restrict__ segs, double* __restrict__ partial) {
  __shared__ double red[256];
  const TrainSeg sg = segs[blockIdx.x];
  double a = 0.0;
  for (unsigned i = threadIdx.x; i < sg.n; i += 256) {
    const double g = (double)sg.g[i];
    a += g * g;
  }
  a = block_sum(a, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = a;
}

__global__ __launch_bounds__(256) void k_sqnorm_final(const double* __restrict__ partial, int n, double* __restrict__ out) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += partial[i];
  a = block_sum(a, red);
  if (threadIdx.x == 0) out[0] = a;
}

// torch.optim.AdamW (single tensor): p *= 1 - lr wd; m.lerp_(g, 1 - b1); v = v b2 + (1 - b2) g g;
// p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps); g is the gradient times the clip coefficient.
struct AdamScalars {
  float decay, w1, b2, w2, bc2_sqrt, eps, step_size;
  double max_norm;  // <= 0: no clipping
};
__device__ __forceinline__ float clip_coef(const double* sqnorm, double max_norm) {
  if (!sqnorm || !(max_norm > 0.0)) return 1.0f;
  const double c = max_norm / (sqrt(sqnorm[0]) + 1e-6);  // torch.nn.utils.clip_grad_norm_
  return (float)(c < 1.0 ? c : 1.0);
}
__device__ __forceinline__ void adamw_elem(float* p, const float* g, float* m, float* v, unsigned i, float coef,
                                           const AdamScalars& S) {
  const float gr = g[i] * coef;
  float pp = p[i] * S.decay;
  const float mm = m[i] + (gr - m[i]) * S.w1;
  const float vv = v[i] * S.b2 + (S.w2 * gr) * gr;
  const float denom = sqrtf(vv) / S.bc2_sqrt + S.eps;
  pp = pp - S.step_size * (mm / denom);
  p[i] = pp, m[i] = mm, v[i] = vv;
}
__global__ __launch_bounds__(256) void k_adamw_seg(const TrainSeg* __restrict__ segs, const double* __restrict__ sqnorm,
                                                   AdamScalars S) {
  const TrainSeg sg = segs[blockIdx.x];
  const float coef = clip_coef(sqnorm, S.max_norm);
  for (unsigned i = threadIdx.x; i < sg.n; i += 256) adamw_elem(sg.p, sg.g, sg.m, sg.v, i, coef, S);
}
__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, size_t n, const double* __restrict__ sqnorm,
                                               AdamScalars S) {
  const float coef = clip_coef(sqnorm, S.max_norm);
  const size_t seg = (size_t)blockIdx.x * TRAIN_SEG;
  const unsigned cnt = (unsigned)(n - seg < TRAIN_SEG ? n - seg : TRAIN_SEG);
  for (unsigned i = threadIdx.x; i < cnt; i += 256) adamw_elem(p + seg, g + seg, m + seg, v + seg, i, coef, S);
}

static int adam_scalars(const ffd_adamw_cfg* c, AdamScalars* S) {
  if (!c || c->step < 1 || !(c->lr >= 0.0) || !(c->beta1 >= 0.0 && c->beta1 < 1.0) || !(c->beta2 >= 0.0 && c->beta2 < 1.0) ||
      !(c->eps >= 0.0) || !(c->weight_decay >= 0.0) || !isfinite(c->lr) || !isfinite(c->max_norm))
    return FFD_ERR_INVALID;
  const double bc1 = 1.0 - pow(c->beta1, (double)c->step), bc2 = 1.0 - pow(c->beta2, (double)c->step);
  S->decay = (float)(1.0 - c->lr * c->weight_decay);
  S->w1 = (float)(1.0 - c->beta1);
  S->b2 = (float)c->beta2;
  S->w2 = (float)(1.0 - c->beta2);
  S->bc2_sqrt = (float)sqrt(bc2);
  S->eps = (float)c->eps;
  S->step_size = (float)(c->lr / bc1);
  S->max_norm = c->max_norm;
  return FFD_OK;
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): the context-free operators ------------------------------------------------------------------
using namespace ffd;

static int gemm_shape_ok(int M, int N, int K) {
  if (M < 1 || N < 1 || K < 1) return FFD_ERR_INVALID;
  if ((double)M * N >= 2147483648.0 || (double)M * K >= 2147483648.0 || (double)N * K >= 2147483648.0)
    return FFD_ERR_UNSUPPORTED;
  // N and K tiles lie on grid.y / grid.z-free axes limited to 65 535 workgroups (M lies on grid.x of dgrad, in chunks of wgrad)
  if (cdiv(N, TG_TILE) > 65535 || cdiv(K, TG_TILE) > 65535) return FFD_ERR_UNSUPPORTED;
  return FFD_OK;
}

extern "C" {

int ffd_dense_dgrad(const float* dY, const float* W, const float* act, const float* R, float* dX, int M, int N, int K,
                    void* stream) {
  if (!dY || !W || !dX || dX == dY) return FFD_ERR_INVALID;
  if (int rc = gemm_shape_ok(M, N, K)) return rc;
  return launch_dense_dgrad(dY, W, act, R, dX, M, N, K, (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_dense_wgrad_chunks(int M, int N, int K) { return gemm_shape_ok(M, N, K) == FFD_OK ? wgrad_plan(M, N, K).nchunks : 0; }

size_t ffd_dense_wgrad_work_bytes(int M, int N, int K) {
  return gemm_shape_ok(M, N, K) == FFD_OK ? wgrad_work_bytes(M, N, K) : 0;
}

int ffd_dense_wgrad(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, void* work,
                    size_t work_bytes, void* stream) {
  if (!dY || !X || !dW) return FFD_ERR_INVALID;
  if (int rc = gemm_shape_ok(M, N, K)) return rc;
  const size_t need = wgrad_work_bytes(M, N, K);
  if (need && (!work || work_bytes < need || (reinterpret_cast<uintptr_t>(work) & 7))) return FFD_ERR_INVALID;
  return launch_dense_wgrad(dY, X, dW, db, M, N, K, work, (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_sm_loss_grad(const float* score, const float* sigma, const float* G, const float* z, uint64_t seed,
                     uint64_t sample_offset, const int64_t* index, int likelihood_weighting, double* per_sample_out,
                     float* dscore, int B, int L, int C, void* stream) {
  if (!score || !sigma || !G || !per_sample_out || !dscore) return FFD_ERR_INVALID;
  if (B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  if ((double)L * C >= 2147483648.0) return FFD_ERR_UNSUPPORTED;
  return launch_sm_loss_grad(score, sigma, G, z, seed, sample_offset, index, likelihood_weighting, per_sample_out, dscore,
                             B, L, C, (hipStream_t)stream) == hipSuccess
             ? FFD_OK
             : FFD_ERR_HIP;
}

int ffd_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const double* sqnorm,
              const ffd_adamw_cfg* cfg, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n < 1) return FFD_ERR_INVALID;
  AdamScalars S;
  if (int rc = adam_scalars(cfg, &S)) return rc;
  if (n > (size_t)TRAIN_SEG * 0x7FFFFFFFu) return FFD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_adamw, dim3((unsigned)((n + TRAIN_SEG - 1) / TRAIN_SEG)), dim3(256), 0, (hipStream_t)stream, param,
                     grad, exp_avg, exp_avg_sq, n, sqnorm, S);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

// transformers.get_cosine_schedule_with_warmup's factor times lr_max (score_models.py:318-324)
double ffd_host_lr_schedule(double lr_max, long long step, long long num_warmup_steps, long long num_training_steps) {
  if (step < num_warmup_steps) return lr_max * (double)step / (double)(num_warmup_steps > 1 ? num_warmup_steps : 1);
  const long long span = num_training_steps - num_warmup_steps;
  const double progress = (double)(step - num_warmup_steps) / (double)(span > 1 ? span : 1);
  const double f = 0.5 * (1.0 + cos(3.14159265358979323846 * progress));
  return lr_max * (f > 0.0 ? f : 0.0);
}

}  // extern "C"

// ---- the training object ------------------------------------------------------------------------------------------------
namespace {

struct TrainTensor {
  std::string key;
  size_t n;
  bool frozen;  // time_encoder.W (requires_grad=False): no gradient, no decay, no update
  float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;
};

// offsets (in floats) of the MLP's workspace at batch B; every block starts on a multiple of 4 floats
struct MlpWork {
  size_t xn, tb, sgb, emb, temb, h, u, score, dscore, dh0, dh1, du, wg, total_bytes;
};
static size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }
static MlpWork mlp_work(const ffd_model_desc& m, int B) {
  const size_t io = (size_t)m.max_len * m.n_channels, d = m.d_model, F = m.dim_feedforward, NL = m.num_layers, b = B;
  MlpWork w;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += up4(n); return at; };
  w.xn = take(b * io), w.tb = take(b), w.sgb = take(b), w.emb = take(b * d), w.temb = take(b * d);
  w.h = take((NL + 1) * b * d), w.u = take(NL * b * F), w.score = take(b * io), w.dscore = take(b * io);
  w.dh0 = take(b * d), w.dh1 = take(b * d), w.du = take(b * F);
  size_t wg = wgrad_work_bytes(B, (int)io, (int)d);  // the largest product N K of the model's wgrads
  wg = std::max(wg, wgrad_work_bytes(B, (int)d, (int)io));
  wg = std::max(wg, wgrad_work_bytes(B, (int)F, (int)d));
  wg = std::max(wg, wgrad_work_bytes(B, (int)d, (int)F));
  wg = std::max(wg, wgrad_work_bytes(B, (int)d, (int)d));
  w.wg = take((wg + 3) / 4);
  w.total_bytes = o * sizeof(float);
  return w;
}

}  // namespace

struct ffd_train {
  ffd_model_desc desc{};
  int device = 0;
  std::string err;
  std::vector<TrainTensor> t;
  float* G_dev = nullptr;
  float* work = nullptr;
  size_t work_bytes = 0;
  int fwd_B = 0;  // the batch whose activations the workspace holds (ffd_train_input_vjp); 0: none
  TrainSeg* segs = nullptr;  // the bound trainable tensors in segments of TRAIN_SEG, rebuilt after a bind
  int nseg = 0;
  bool segs_stale = true;
  double* partial = nullptr;  // nseg doubles + the squared norm of ffd_train_step
  // classes (ffd_train_classes / ffd_train_labels): the caller's device labels, and the effective labels of the batch in
  // flight (after the dropout) in a buffer of their own -- outside the workspace, whose size the ABI states
  int n_classes = 0;
  const int32_t* labels = nullptr;
  size_t n_labels = 0;
  double p_uncond = 0.0;
  int32_t* eff = nullptr;
  size_t eff_cap = 0;
  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
  TrainTensor* find(const char* key) {
    for (auto& x : t)
      if (x.key == key) return &x;
    return nullptr;
  }
  float* par(const std::string& key) { return find(key.c_str())->p; }
  float* grd(const std::string& key) { return find(key.c_str())->g; }
};

#define TRCHECK(expr)                                                                                                \
  do {                                                                                                               \
    hipError_t e__ = (expr);                                                                                         \
    if (e__ != hipSuccess)                                                                                           \
      return tr->fail(FFD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__);      \
  } while (0)

static int why_fail(std::string* why, int code, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (why) *why = buf;
  return code;
}

static int train_desc_check(const ffd_model_desc* m, double dropout, std::string* why) {
  if (m->n_channels < 1 || m->max_len < 1 || m->num_layers < 1)
    return why_fail(why, FFD_ERR_INVALID, "bad shape: C=%d L=%d NL=%d", m->n_channels, m->max_len, m->num_layers);
  if (!(dropout == 0.0))
    return why_fail(why, FFD_ERR_UNSUPPORTED, "dropout=%g: training runs without dropout only (pass 0.0)", dropout);
  if (m->kind != FFD_MODEL_MLP && m->kind != FFD_MODEL_TRANSFORMER)
    return why_fail(why, FFD_ERR_UNSUPPORTED, "model kind %d has no backward pass (the transformer and the MLP train)", m->kind);
  if (m->d_model < 1 || m->dim_feedforward < 1)
    return why_fail(why, FFD_ERR_INVALID, "d_model=%d dim_feedforward=%d", m->d_model, m->dim_feedforward);
  if (m->kind == FFD_MODEL_TRANSFORMER) {
    if (m->n_head < 1 || m->d_model % m->n_head != 0)
      return why_fail(why, FFD_ERR_INVALID, "d_model=%d not divisible by n_head=%d", m->d_model, m->n_head);
    if (m->d_model / m->n_head > 8 || m->max_len > 512)
      return why_fail(why, FFD_ERR_UNSUPPORTED, "head_dim=%d, max_len=%d: the attention backward takes head_dim <= 8, L <= 512",
                      m->d_model / m->n_head, m->max_len);
  }
  if (m->sde != FFD_SDE_VP && m->sde != FFD_SDE_VE) return why_fail(why, FFD_ERR_UNSUPPORTED, "sde kind %d", m->sde);
  if ((double)m->max_len * m->n_channels >= 2147483648.0) return why_fail(why, FFD_ERR_UNSUPPORTED, "L * C >= 2^31");
  return FFD_OK;
}

static void train_tensors(ffd_train* tr) {
  const ffd_model_desc& m = tr->desc;
  const size_t io = (size_t)m.max_len * m.n_channels, d = m.d_model, F = m.dim_feedforward;
  auto add = [&](const std::string& key, size_t n, bool frozen = false) { tr->t.push_back({key, n, frozen}); };
  add("time_encoder.W", (d + 1) / 2, true);
  add("time_encoder.dense.weight", d * d), add("time_encoder.dense.bias", d);
  if (m.kind == FFD_MODEL_TRANSFORMER) {
    const size_t C = m.n_channels;
    add("pos_encoder.embedding.weight", (size_t)m.max_len * d);
    add("embedder.weight", d * C), add("embedder.bias", d), add("unembedder.weight", C * d), add("unembedder.bias", C);
    for (int i = 0; i < m.num_layers; ++i) {
      const std::string p = "backbone.layers." + std::to_string(i) + ".";
      add(p + "self_attn.in_proj_weight", 3 * d * d), add(p + "self_attn.in_proj_bias", 3 * d);
      add(p + "self_attn.out_proj.weight", d * d), add(p + "self_attn.out_proj.bias", d);
      add(p + "linear1.weight", F * d), add(p + "linear1.bias", F), add(p + "linear2.weight", d * F), add(p + "linear2.bias", d);
      add(p + "norm1.weight", d), add(p + "norm1.bias", d), add(p + "norm2.weight", d), add(p + "norm2.bias", d);
    }
    return;
  }
  add("embedder.weight", d * io), add("embedder.bias", d);
  add("unembedder.weight", io * d), add("unembedder.bias", io);
  for (int i = 0; i < m.num_layers; ++i) {
    const std::string p = "backbone." + std::to_string(i) + ".";
    add(p + "0.weight", F * d), add(p + "0.bias", F), add(p + "3.weight", d * F), add(p + "3.bias", d);
  }
}

static int train_ready(ffd_train* tr) {
  for (const auto& x : tr->t)
    if (!x.p) return tr->fail(FFD_ERR_STATE, "tensor %s is not bound (ffd_train_bind)", x.key.c_str());
  return FFD_OK;
}

// what training adds to train_ready: a trainable tensor bound by ffd_train_bind_params has no gradient and no moments
static int train_trainable(ffd_train* tr) {
  if (int rc = train_ready(tr)) return rc;
  for (const auto& x : tr->t)
    if (!x.frozen && !x.g)
      return tr->fail(FFD_ERR_STATE, "tensor %s is bound without gradient and moments (ffd_train_bind_params): the object "
                      "serves inference only", x.key.c_str());
  return FFD_OK;
}

// The effective labels of a batch of B: labels[index[b] | b], dropped to null with probability p under (seed,
// SM_TAG_CLASS_DROP, global row) -- p = 0 for the plain forward.  Without classes: nothing.
static int train_eff_labels(ffd_train* tr, const int64_t* index, int B, double p, uint64_t seed, uint64_t sample_offset,
                            hipStream_t s) {
  if (!tr->n_classes) return FFD_OK;
  if (!index && tr->labels && tr->n_labels < (size_t)B)
    return tr->fail(FFD_ERR_INVALID, "%zu labels for a batch of %d rows (ffd_train_labels)", tr->n_labels, B);
  if (tr->eff_cap < (size_t)B) {
    if (tr->eff) {
      (void)hipDeviceSynchronize();
      (void)hipFree(tr->eff);
      tr->eff = nullptr, tr->eff_cap = 0;
    }
    if (hipMalloc((void**)&tr->eff, (size_t)B * sizeof(int32_t)) != hipSuccess)
      return tr->fail(FFD_ERR_NOMEM, "hipMalloc(%d labels) failed", B);
    tr->eff_cap = (size_t)B;
  }
  TRCHECK(launch_class_drop(tr->labels, tr->n_classes, index, B, (float)p, seed, sample_offset, tr->eff, s));
  return FFD_OK;
}
// temb (B, d) += table[eff_label_b], in place, behind the time encoder's dense layer
static int train_class_rows(ffd_train* tr, float* temb, int B, hipStream_t s) {
  if (!tr->n_classes) return FFD_OK;
  const int d = tr->desc.d_model;
  TRCHECK(launch_class_temb(temb, d, tr->par("class_embedding.weight"), tr->n_classes, tr->eff, B, d, 0, temb, nullptr, nullptr,
                            0, s));
  return FFD_OK;
}
static int train_class_grad(ffd_train* tr, const float* dtemb, int B, hipStream_t s) {
  if (!tr->n_classes) return FFD_OK;
  TRCHECK(launch_class_table_grad(dtemb, tr->eff, tr->n_classes, B, tr->desc.d_model, tr->grd("class_embedding.weight"), s));
  return FFD_OK;
}

// the transformer's path (behind the LayerNorm and attention operators at the end of this file)
static size_t tf_work_bytes(const ffd_model_desc& m, int B);
static int tf_forward(ffd_train* tr, const float* xn, const float* tb, int B, hipStream_t s);
static int tf_input_vjp(ffd_train* tr, const float* v, float* dx, int B, hipStream_t s);
static int tf_loss_grad(ffd_train* tr, const float* x0, const int64_t* index, const float* timesteps, const float* mean_coeff,
                        const float* sigma, const float* z, uint64_t seed, uint64_t sample_offset, int lw,
                        double* per_sample_out, int B, hipStream_t s);
static const float* tf_score(ffd_train* tr, int B);
static size_t train_work_need(const ffd_model_desc& m, int B) {
  return m.kind == FFD_MODEL_TRANSFORMER ? tf_work_bytes(m, B) : mlp_work(m, B).total_bytes;
}

static int train_workspace(ffd_train* tr, int B) {
  const size_t need = train_work_need(tr->desc, B);
  if (need <= tr->work_bytes) return FFD_OK;
  if (tr->work) {
    (void)hipDeviceSynchronize();
    (void)hipFree(tr->work);
    tr->work = nullptr, tr->work_bytes = 0, tr->fwd_B = 0;
  }
  if (hipMalloc((void**)&tr->work, need + 256) != hipSuccess)
    return tr->fail(FFD_ERR_NOMEM, "hipMalloc(%zu bytes) of the training workspace failed", need);
  tr->work_bytes = need;
  return FFD_OK;
}

// the segment table of the bound trainable tensors, in the order of train_tensors (one blocking copy after a bind)
static int train_segments(ffd_train* tr) {
  if (!tr->segs_stale) return FFD_OK;
  std::vector<TrainSeg> host;
  for (const auto& x : tr->t) {
    if (x.frozen) continue;
    for (size_t o = 0; o < x.n; o += TRAIN_SEG)
      host.push_back({x.p + o, x.g + o, x.m + o, x.v + o, (unsigned)std::min<size_t>(TRAIN_SEG, x.n - o), 0u});
  }
  (void)hipDeviceSynchronize();
  if (tr->segs) (void)hipFree(tr->segs);
  if (tr->partial) (void)hipFree(tr->partial);
  tr->segs = nullptr, tr->partial = nullptr;
  TRCHECK(hipMalloc((void**)&tr->segs, host.size() * sizeof(TrainSeg)));
  TRCHECK(hipMalloc((void**)&tr->partial, (host.size() + 1) * sizeof(double)));
  TRCHECK(hipMemcpy(tr->segs, host.data(), host.size() * sizeof(TrainSeg), hipMemcpyHostToDevice));
  tr->nseg = (int)host.size();
  tr->segs_stale = false;
  return FFD_OK;
}

// MLPScoreModule.forward (score_models.py:406-440) keeping every layer's input h_i and hidden activation u_i
static int mlp_train_forward(ffd_train* tr, const float* xn, const float* tb, const MlpWork& w, int B, hipStream_t s) {
  const ffd_model_desc& m = tr->desc;
  const int io = m.max_len * m.n_channels, d = m.d_model, F = m.dim_feedforward, NL = m.num_layers;
  float* W = tr->work;
  hipLaunchKernelGGL(k_time_features, dim3(cdiv(B * d, 256)), dim3(256), 0, s, tb, tr->par("time_encoder.W"), W + w.emb, B, d);
  TRCHECK(hipGetLastError());
  TRCHECK(launch_dense(W + w.emb, tr->par("time_encoder.dense.weight"), tr->par("time_encoder.dense.bias"), nullptr, nullptr,
                       W + w.temb, B, d, d, 0, s));
  if (int rc = train_class_rows(tr, W + w.temb, B, s)) return rc;
  TRCHECK(launch_dense(xn, tr->par("embedder.weight"), tr->par("embedder.bias"), nullptr, W + w.temb, W + w.h, B, d, io, 0, s));
  for (int i = 0; i < NL; ++i) {
    const std::string p = "backbone." + std::to_string(i) + ".";
    float *hi = W + w.h + (size_t)i * B * d, *ui = W + w.u + (size_t)i * B * F;
    TRCHECK(launch_dense(hi, tr->par(p + "0.weight"), tr->par(p + "0.bias"), nullptr, nullptr, ui, B, F, d, 1, s));
    TRCHECK(launch_dense(ui, tr->par(p + "3.weight"), tr->par(p + "3.bias"), nullptr, hi, hi + (size_t)B * d, B, d, F, 0, s));
  }
  TRCHECK(launch_dense(W + w.h + (size_t)NL * B * d, tr->par("unembedder.weight"), tr->par("unembedder.bias"), nullptr, nullptr,
                       W + w.score, B, io, d, 0, s));
  return FFD_OK;
}

static int mlp_train_backward(ffd_train* tr, const MlpWork& w, int B, hipStream_t s) {
  const ffd_model_desc& m = tr->desc;
  const int io = m.max_len * m.n_channels, d = m.d_model, F = m.dim_feedforward, NL = m.num_layers;
  float* W = tr->work;
  void* wg = W + w.wg;
  float *dh = W + w.dh0, *dh_alt = W + w.dh1;
  const float* hN = W + w.h + (size_t)NL * B * d;
  TRCHECK(launch_dense_wgrad(W + w.dscore, hN, tr->grd("unembedder.weight"), tr->grd("unembedder.bias"), B, io, d, wg, s));
  TRCHECK(launch_dense_dgrad(W + w.dscore, tr->par("unembedder.weight"), nullptr, nullptr, dh, B, io, d, s));
  for (int i = NL - 1; i >= 0; --i) {
    const std::string p = "backbone." + std::to_string(i) + ".";
    const float *hi = W + w.h + (size_t)i * B * d, *ui = W + w.u + (size_t)i * B * F;
    TRCHECK(launch_dense_wgrad(dh, ui, tr->grd(p + "3.weight"), tr->grd(p + "3.bias"), B, d, F, wg, s));
    TRCHECK(launch_dense_dgrad(dh, tr->par(p + "3.weight"), ui, nullptr, W + w.du, B, d, F, s));
    TRCHECK(launch_dense_wgrad(W + w.du, hi, tr->grd(p + "0.weight"), tr->grd(p + "0.bias"), B, F, d, wg, s));
    TRCHECK(launch_dense_dgrad(W + w.du, tr->par(p + "0.weight"), nullptr, dh, dh_alt, B, F, d, s));  // + the residual path
    std::swap(dh, dh_alt);
  }
  TRCHECK(launch_dense_wgrad(dh, W + w.xn, tr->grd("embedder.weight"), tr->grd("embedder.bias"), B, d, io, wg, s));
  TRCHECK(launch_dense_wgrad(dh, W + w.emb, tr->grd("time_encoder.dense.weight"), tr->grd("time_encoder.dense.bias"), B, d, d,
                             wg, s));
  return train_class_grad(tr, dh, B, s);  // (the (B, d) state's gradient is the time embedding's)
}

// The MLP's backward chain for the input alone: no wgrad, and one more dgrad through embedder.weight
static int mlp_input_vjp(ffd_train* tr, const float* v, float* dx, const MlpWork& w, int B, hipStream_t s) {
  const ffd_model_desc& m = tr->desc;
  const int io = m.max_len * m.n_channels, d = m.d_model, F = m.dim_feedforward, NL = m.num_layers;
  float* W = tr->work;
  float *dh = W + w.dh0, *dh_alt = W + w.dh1;
  TRCHECK(launch_dense_dgrad(v, tr->par("unembedder.weight"), nullptr, nullptr, dh, B, io, d, s));
  for (int i = NL - 1; i >= 0; --i) {
    const std::string p = "backbone." + std::to_string(i) + ".";
    const float* ui = W + w.u + (size_t)i * B * F;
    TRCHECK(launch_dense_dgrad(dh, tr->par(p + "3.weight"), ui, nullptr, W + w.du, B, d, F, s));
    TRCHECK(launch_dense_dgrad(W + w.du, tr->par(p + "0.weight"), nullptr, dh, dh_alt, B, F, d, s));  // + the residual path
    std::swap(dh, dh_alt);
  }
  TRCHECK(launch_dense_dgrad(dh, tr->par("embedder.weight"), nullptr, nullptr, dx, B, d, io, s));
  return FFD_OK;
}

static int train_loss_grad(ffd_train* tr, const float* x0, const int64_t* index, const float* timesteps,
                           const float* mean_coeff, const float* sigma, const float* z, uint64_t seed,
                           uint64_t sample_offset, int lw, double* per_sample_out, int B, hipStream_t s) {
  const ffd_model_desc& m = tr->desc;
  TRCHECK(hipSetDevice(tr->device));
  if (int rc = train_workspace(tr, B)) return rc;
  tr->fwd_B = 0;  // (B again once everything is enqueued: the forward's activations are what ffd_train_input_vjp reads)
  if (int rc = train_eff_labels(tr, index, B, tr->p_uncond, seed, sample_offset, s)) return rc;
  if (m.kind == FFD_MODEL_TRANSFORMER) {
    if (int rc = tf_loss_grad(tr, x0, index, timesteps, mean_coeff, sigma, z, seed, sample_offset, lw, per_sample_out, B, s))
      return rc;
    tr->fwd_B = B;
    return FFD_OK;
  }
  const MlpWork w = mlp_work(m, B);
  float* W = tr->work;
  hipLaunchKernelGGL(k_train_perturb, dim3((unsigned)B), dim3(256), 0, s, x0, W + w.xn, timesteps, mean_coeff, sigma,
                     tr->G_dev, z, seed, sample_offset, index, W + w.tb, W + w.sgb, (unsigned)m.max_len,
                     (unsigned)m.n_channels);
  TRCHECK(hipGetLastError());
  if (int rc = mlp_train_forward(tr, W + w.xn, W + w.tb, w, B, s)) return rc;
  TRCHECK(launch_sm_loss_grad(W + w.score, W + w.sgb, tr->G_dev, z, seed, sample_offset, index, lw, per_sample_out,
                              W + w.dscore, B, m.max_len, m.n_channels, s));
  if (int rc = mlp_train_backward(tr, w, B, s)) return rc;
  tr->fwd_B = B;
  return FFD_OK;
}

static int train_batch_args(ffd_train* tr, const float* x0, const float* timesteps, const float* mean_coeff,
                            const float* sigma, double* per_sample_out, int B) {
  if (!x0 || !timesteps || !mean_coeff || !sigma || !per_sample_out) return tr->fail(FFD_ERR_INVALID, "null buffer");
  if (B < 1) return tr->fail(FFD_ERR_INVALID, "B=%d", B);
  if ((double)B * tr->desc.max_len * tr->desc.n_channels >= 2147483648.0 ||
      (double)B * tr->desc.dim_feedforward * (tr->desc.kind == FFD_MODEL_TRANSFORMER ? tr->desc.max_len : 1) >= 2147483648.0 ||
      (double)B * tr->desc.max_len * tr->desc.d_model * 3 >= 2147483648.0)
    return tr->fail(FFD_ERR_UNSUPPORTED, "B=%d: a batch's activations are indexed in 32 bits", B);
  return train_trainable(tr);
}

namespace ffd {
const ffd_model_desc& train_desc(const ffd_train* tr) { return tr->desc; }
}  // namespace ffd

extern "C" {

int ffd_train_create(ffd_train** out, const ffd_model_desc* desc, double dropout, int device) {
  if (!out || !desc) return FFD_ERR_INVALID;
  ffd_train* tr = new ffd_train();
  tr->desc = *desc;
  tr->device = device;
  *out = tr;  // returned even on failure so the caller can read the message
  if (int rc = train_desc_check(desc, dropout, &tr->err)) return rc;
  train_tensors(tr);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return tr->fail(FFD_ERR_HIP, "no HIP device available (%s): libffd has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return tr->fail(FFD_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
  TRCHECK(hipSetDevice(device));
  std::vector<float> G(desc->max_len);
  ffd_host_noise_scaling(desc->max_len, desc->fourier_noise_scaling, G.data());
  TRCHECK(hipMalloc((void**)&tr->G_dev, sizeof(float) * G.size()));
  TRCHECK(hipMemcpy(tr->G_dev, G.data(), sizeof(float) * G.size(), hipMemcpyHostToDevice));
  return FFD_OK;
}

void ffd_train_destroy(ffd_train* tr) {
  if (!tr) return;
  if (tr->G_dev || tr->work || tr->segs || tr->partial || tr->eff) {
    (void)hipSetDevice(tr->device);
    (void)hipDeviceSynchronize();
    for (void* p : {(void*)tr->G_dev, (void*)tr->work, (void*)tr->segs, (void*)tr->partial, (void*)tr->eff})
      if (p) (void)hipFree(p);
  }
  delete tr;
}

const char* ffd_train_last_error(const ffd_train* tr) { return tr ? tr->err.c_str() : "null training object"; }

size_t ffd_train_work_bytes(const ffd_model_desc* desc, int B) {
  if (!desc || B < 1 || train_desc_check(desc, 0.0, nullptr) != FFD_OK) return 0;
  return train_work_need(*desc, B);
}

int ffd_train_classes(ffd_train* tr, int n_classes) {
  if (!tr) return FFD_ERR_INVALID;
  if (n_classes < 1) return tr->fail(FFD_ERR_INVALID, "n_classes=%d", n_classes);
  if (tr->n_classes) return tr->fail(FFD_ERR_INVALID, "the object already has %d classes", tr->n_classes);
  if (tr->t.empty()) return tr->fail(FFD_ERR_STATE, "the object was not created (ffd_train_create failed)");
  for (const auto& x : tr->t)
    if (x.p) return tr->fail(FFD_ERR_STATE, "ffd_train_classes comes before the first bind (%s is bound)", x.key.c_str());
  tr->t.push_back({"class_embedding.weight", ((size_t)n_classes + 1) * (size_t)tr->desc.d_model, false});
  tr->n_classes = n_classes;
  tr->segs_stale = true;
  return FFD_OK;
}

int ffd_train_labels(ffd_train* tr, const int32_t* labels, size_t n, double p_uncond) {
  if (!tr) return FFD_ERR_INVALID;
  if (!tr->n_classes) return tr->fail(FFD_ERR_STATE, "ffd_train_labels without ffd_train_classes");
  if (labels && n < 1) return tr->fail(FFD_ERR_INVALID, "labels of length 0");
  if (!(p_uncond >= 0.0 && p_uncond <= 1.0)) return tr->fail(FFD_ERR_INVALID, "p_uncond=%g outside [0, 1]", p_uncond);
  tr->labels = labels, tr->n_labels = labels ? n : 0, tr->p_uncond = p_uncond;
  return FFD_OK;
}

int ffd_train_bind(ffd_train* tr, const char* name, float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n) {
  if (!tr) return FFD_ERR_INVALID;
  if (!name || !param) return tr->fail(FFD_ERR_INVALID, "null name or parameter");
  TrainTensor* x = tr->find(name);
  if (!x) return tr->fail(FFD_ERR_INVALID, "unknown tensor %s", name);
  if (n != x->n) return tr->fail(FFD_ERR_INVALID, "%s has %zu elements, the model takes %zu", name, n, x->n);
  if (!x->frozen && (!grad || !exp_avg || !exp_avg_sq))
    return tr->fail(FFD_ERR_INVALID, "%s needs its gradient and both moments", name);
  x->p = param;
  x->g = x->frozen ? nullptr : grad, x->m = x->frozen ? nullptr : exp_avg, x->v = x->frozen ? nullptr : exp_avg_sq;
  tr->segs_stale = true;
  return FFD_OK;
}

int ffd_train_bind_params(ffd_train* tr, const char* name, float* param, size_t n) {
  if (!tr) return FFD_ERR_INVALID;
  if (!name || !param) return tr->fail(FFD_ERR_INVALID, "null name or parameter");
  TrainTensor* x = tr->find(name);
  if (!x) return tr->fail(FFD_ERR_INVALID, "unknown tensor %s", name);
  if (n != x->n) return tr->fail(FFD_ERR_INVALID, "%s has %zu elements, the model takes %zu", name, n, x->n);
  x->p = param;
  x->g = x->m = x->v = nullptr;
  tr->segs_stale = true;
  return FFD_OK;
}

int ffd_train_forward(ffd_train* tr, const float* x, const float* timesteps, float* score_out, int B, void* stream) {
  if (!tr) return FFD_ERR_INVALID;
  if (!x || !timesteps || !score_out) return tr->fail(FFD_ERR_INVALID, "null buffer");
  if (B < 1) return tr->fail(FFD_ERR_INVALID, "B=%d", B);
  if (int rc = train_ready(tr)) return rc;
  TRCHECK(hipSetDevice(tr->device));
  if (int rc = train_workspace(tr, B)) return rc;
  tr->fwd_B = 0;  // (B again once the forward is enqueued)
  hipStream_t s = (hipStream_t)stream;
  if (int rc = train_eff_labels(tr, nullptr, B, 0.0, 0, 0, s)) return rc;
  if (tr->desc.kind == FFD_MODEL_TRANSFORMER) {
    if (int rc = tf_forward(tr, x, timesteps, B, s)) return rc;
    TRCHECK(hipMemcpyAsync(score_out, tf_score(tr, B), sizeof(float) * (size_t)B * tr->desc.max_len * tr->desc.n_channels,
                           hipMemcpyDeviceToDevice, s));
    tr->fwd_B = B;
    return FFD_OK;
  }
  const MlpWork w = mlp_work(tr->desc, B);
  if (int rc = mlp_train_forward(tr, x, timesteps, w, B, s)) return rc;
  TRCHECK(hipMemcpyAsync(score_out, tr->work + w.score, sizeof(float) * (size_t)B * tr->desc.max_len * tr->desc.n_channels,
                         hipMemcpyDeviceToDevice, s));
  tr->fwd_B = B;
  return FFD_OK;
}

int ffd_train_input_vjp(ffd_train* tr, const float* v, float* dx_out, int B, void* stream) {
  if (!tr) return FFD_ERR_INVALID;
  if (!v || !dx_out || v == dx_out) return tr->fail(FFD_ERR_INVALID, "null or aliased buffer");
  if (B < 1) return tr->fail(FFD_ERR_INVALID, "B=%d", B);
  if (int rc = train_ready(tr)) return rc;
  if (tr->fwd_B != B)
    return tr->fail(FFD_ERR_STATE, "ffd_train_input_vjp at B=%d: the workspace holds %s", B,
                    tr->fwd_B ? "the activations of another batch size" : "no forward's activations");
  TRCHECK(hipSetDevice(tr->device));
  if (tr->desc.kind == FFD_MODEL_TRANSFORMER) return tf_input_vjp(tr, v, dx_out, B, (hipStream_t)stream);
  return mlp_input_vjp(tr, v, dx_out, mlp_work(tr->desc, B), B, (hipStream_t)stream);
}

int ffd_train_loss_grad(ffd_train* tr, const float* x0, const int64_t* index, const float* timesteps,
                        const float* mean_coeff, const float* sigma, const float* z, uint64_t seed, uint64_t sample_offset,
                        int likelihood_weighting, double* per_sample_out, int B, void* stream) {
  if (!tr) return FFD_ERR_INVALID;
  if (int rc = train_batch_args(tr, x0, timesteps, mean_coeff, sigma, per_sample_out, B)) return rc;
  return train_loss_grad(tr, x0, index, timesteps, mean_coeff, sigma, z, seed, sample_offset, likelihood_weighting,
                         per_sample_out, B, (hipStream_t)stream);
}

int ffd_train_grad_sqnorm(ffd_train* tr, double* sqnorm_out, void* stream) {
  if (!tr) return FFD_ERR_INVALID;
  if (!sqnorm_out) return tr->fail(FFD_ERR_INVALID, "null buffer");
  if (int rc = train_trainable(tr)) return rc;
  TRCHECK(hipSetDevice(tr->device));
  if (int rc = train_segments(tr)) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sqnorm_seg, dim3(tr->nseg), dim3(256), 0, s, tr->segs, tr->partial);
  hipLaunchKernelGGL(k_sqnorm_final, dim3(1), dim3(256), 0, s, tr->partial, tr->nseg, sqnorm_out);
  TRCHECK(hipGetLastError());
  return FFD_OK;
}

int ffd_train_adamw(ffd_train* tr, const double* sqnorm, const ffd_adamw_cfg* cfg, void* stream) {
  if (!tr) return FFD_ERR_INVALID;
  AdamScalars S;
  if (adam_scalars(cfg, &S)) return tr->fail(FFD_ERR_INVALID, "bad AdamW configuration");
  if (cfg->max_norm > 0.0 && !sqnorm) return tr->fail(FFD_ERR_INVALID, "clipping needs the squared gradient norm");
  if (int rc = train_trainable(tr)) return rc;
  TRCHECK(hipSetDevice(tr->device));
  if (int rc = train_segments(tr)) return rc;
  tr->fwd_B = 0;  // the parameters move: the activations a forward kept are no longer theirs (ffd_train_input_vjp)
  hipLaunchKernelGGL(k_adamw_seg, dim3(tr->nseg), dim3(256), 0, (hipStream_t)stream, tr->segs, sqnorm, S);
  TRCHECK(hipGetLastError());
  return FFD_OK;
}

int ffd_train_step(ffd_train* tr, const float* x0, const int64_t* index, const float* timesteps, const float* mean_coeff,
                   const float* sigma, const float* z, uint64_t seed, uint64_t sample_offset, int likelihood_weighting,
                   double* per_sample_out, int B, const ffd_adamw_cfg* cfg, void* stream) {
  if (!tr) return FFD_ERR_INVALID;
  AdamScalars S;
  if (adam_scalars(cfg, &S)) return tr->fail(FFD_ERR_INVALID, "bad AdamW configuration");
  if (int rc = train_batch_args(tr, x0, timesteps, mean_coeff, sigma, per_sample_out, B)) return rc;
  TRCHECK(hipSetDevice(tr->device));
  if (int rc = train_segments(tr)) return rc;
  if (int rc = train_loss_grad(tr, x0, index, timesteps, mean_coeff, sigma, z, seed, sample_offset, likelihood_weighting,
                               per_sample_out, B, (hipStream_t)stream))
    return rc;
  tr->fwd_B = 0;  // the update below moves the parameters: the kept activations are no longer theirs
  double* sq = tr->partial + tr->nseg;
  if (int rc = ffd_train_grad_sqnorm(tr, sq, stream)) return rc;
  return ffd_train_adamw(tr, sq, cfg, stream);
}

}  // extern "C"

// ---- the transformer's operators (its training forward and backward, at the end of this file, chain them) ----------------
// LayerNorm that keeps its statistics, its backward, and attention for head_dim <= 8, L <= 512 on the vector pipe: with
// heads this small a score is a handful of FMAs.  qkv is the in-projection's row-major output (B L, 3 H hd): q | k | v,
// head h at columns h hd of each third; out and its gradient are (B L, H hd); lse is (B, H, L).
namespace ffd {

// losses.py:60-63 for the rows index[b]: the draw ffd_sm_draw_times makes for global sample sample_offset + index[b]
__global__ __launch_bounds__(256) void k_sm_draw_times_at(float* __restrict__ t, const int64_t* __restrict__ index, int B,
                                                          float span, float eps, float T, uint64_t seed,
                                                          uint64_t sample_offset) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const uint64_t g = sample_offset + (uint64_t)index[i];
  const U4 c = {(uint32_t)(g >> 2), (uint32_t)(g >> 34), SM_TAG_TIMES, 0x46464446u};
  const U4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int sl = (int)(g & 3);
  const uint32_t w = sl == 0 ? r.x : sl == 1 ? r.y : sl == 2 ? r.z : r.w;
  const float u = (float)(w >> 8) * (1.0f / 16777216.0f);
  t[i] = fminf(__fadd_rn(__fmul_rn(u, span), eps), T);
}

__device__ __forceinline__ float wave_sum(float v) {  // fixed-order butterfly: every lane gets the same total
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one wave per row: y = xhat gamma + beta, xhat = (x - mean) rstd, rstd = 1 / sqrt(var + eps) (biased variance)
__global__ __launch_bounds__(256) void k_ln_stats_fwd(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ y,
                                                      float* __restrict__ xhat, float* __restrict__ rstd, int M, int D,
                                                      float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* xr = x + (size_t)row * D;
  float s = 0.f;
  for (int j = lane; j < D; j += 64) s += xr[j];
  const float mean = wave_sum(s) / (float)D;
  float v = 0.f;
  for (int j = lane; j < D; j += 64) {
    const float c = xr[j] - mean;
    v += c * c;
  }
  const float rs = 1.0f / sqrtf(wave_sum(v) / (float)D + eps);
  for (int j = lane; j < D; j += 64) {
    const float h = (xr[j] - mean) * rs;
    xhat[(size_t)row * D + j] = h;
    y[(size_t)row * D + j] = h * gamma[j] + beta[j];
  }
  if (lane == 0) rstd[row] = rs;
}

// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; one wave per row
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                float* __restrict__ dx, int M, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const size_t o = (size_t)row * D;
  float a = 0.f, b = 0.f;
  for (int j = lane; j < D; j += 64) {
    const float g = dy[o + j] * gamma[j];
    a += g;
    b += g * xhat[o + j];
  }
  const float m1 = wave_sum(a) / (float)D, m2 = wave_sum(b) / (float)D, rs = rstd[row];
  for (int j = lane; j < D; j += 64) dx[o + j] = rs * (dy[o + j] * gamma[j] - m1 - xhat[o + j] * m2);
}

// dgamma[j] = sum_m dy xhat, dbeta[j] = sum_m dy: one workgroup per column, fp64, rows in a fixed order
__global__ __launch_bounds__(256) void k_ln_param_grad(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta, int M, int D) {
  __shared__ double red[256];
  const int j = blockIdx.x;
  double a = 0.0, b = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) {
    const double g = (double)dy[(size_t)m * D + j];
    a += g * (double)xhat[(size_t)m * D + j];
    b += g;
  }
  a = block_sum(a, red);
  b = block_sum(b, red);
  if (threadIdx.x == 0) dgamma[j] = (float)a, dbeta[j] = (float)b;
}

constexpr int AT_MAX_L = 512, AT_HD = 8;  // rows of one head in LDS, padded to 8 features

__device__ __forceinline__ float dot8(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < AT_HD; ++c) s = fmaf(a[c], b[c], s);
  return s;
}
// rows [0, L) of one third (`sec` 0 q | 1 k | 2 v, or a (B L, d) array with stride d) of head h into an [L][8] image
__device__ __forceinline__ void load_head(float* img, const float* base, size_t stride, int col0, int L, int hd) {
  for (int e = threadIdx.x; e < L * AT_HD; e += 256) {
    const int j = e >> 3, c = e & 7;
    img[e] = c < hd ? base[(size_t)j * stride + col0 + c] : 0.f;
  }
}

// one workgroup per (sample, head); a thread owns query rows tid, tid + 256
__global__ __launch_bounds__(256) void k_attn_lse_fwd(const float* __restrict__ qkv, float* __restrict__ out,
                                                      float* __restrict__ lse, int L, int H, int hd) {
  __shared__ float sK[AT_MAX_L * AT_HD], sV[AT_MAX_L * AT_HD];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, d = H * hd;
  const float* rows = qkv + (size_t)b * L * 3 * d;
  const float scale = 1.0f / sqrtf((float)hd);
  load_head(sK, rows, 3 * d, d + h * hd, L, hd);
  load_head(sV, rows, 3 * d, 2 * d + h * hd, L, hd);
  __syncthreads();
  for (int i = threadIdx.x; i < L; i += 256) {
    float q[AT_HD], o[AT_HD];
#pragma unroll
    for (int c = 0; c < AT_HD; ++c) q[c] = c < hd ? rows[(size_t)i * 3 * d + h * hd + c] : 0.f, o[c] = 0.f;
    float mx = -INFINITY;
    for (int j = 0; j < L; ++j) mx = fmaxf(mx, dot8(q, sK + j * AT_HD) * scale);
    float sum = 0.f;
    for (int j = 0; j < L; ++j) {
      const float p = expf(dot8(q, sK + j * AT_HD) * scale - mx);
      sum += p;
#pragma unroll
      for (int c = 0; c < AT_HD; ++c) o[c] = fmaf(p, sV[j * AT_HD + c], o[c]);
    }
    for (int c = 0; c < hd; ++c) out[((size_t)b * L + i) * d + h * hd + c] = o[c] / sum;
    lse[((size_t)b * H + h) * L + i] = mx + logf(sum);
  }
}

// Query-major pass (K, V in LDS): p from the saved log-sum-exp, D_i = sum_j p dP = dO_i . O_i, dQ.  Key-major pass (Q, dO,
// D, lse in LDS): dK, dV.  Every element of dqkv is written once, by the thread that owns its row.
__global__ __launch_bounds__(256) void k_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ out,
                                                  const float* __restrict__ dout, const float* __restrict__ lse,
                                                  float* __restrict__ dqkv, int L, int H, int hd) {
  __shared__ float sA[AT_MAX_L * AT_HD], sB[AT_MAX_L * AT_HD], sD[AT_MAX_L], sL[AT_MAX_L];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, d = H * hd;
  const float* rows = qkv + (size_t)b * L * 3 * d;
  float* drows = dqkv + (size_t)b * L * 3 * d;
  const float scale = 1.0f / sqrtf((float)hd);
  load_head(sA, rows, 3 * d, d + h * hd, L, hd);      // K
  load_head(sB, rows, 3 * d, 2 * d + h * hd, L, hd);  // V
  __syncthreads();
  for (int i = threadIdx.x; i < L; i += 256) {
    float q[AT_HD], go[AT_HD], dq[AT_HD];
    float D = 0.f;
    const size_t orow = ((size_t)b * L + i) * d + h * hd;
#pragma unroll
    for (int c = 0; c < AT_HD; ++c) {
      q[c] = c < hd ? rows[(size_t)i * 3 * d + h * hd + c] : 0.f;
      go[c] = c < hd ? dout[orow + c] : 0.f;
      D = fmaf(go[c], c < hd ? out[orow + c] : 0.f, D);
      dq[c] = 0.f;
    }
    const float l = lse[((size_t)b * H + h) * L + i];
    sD[i] = D, sL[i] = l;
    for (int j = 0; j < L; ++j) {
      const float p = expf(dot8(q, sA + j * AT_HD) * scale - l);
      const float dS = p * (dot8(go, sB + j * AT_HD) - D);
#pragma unroll
      for (int c = 0; c < AT_HD; ++c) dq[c] = fmaf(dS, sA[j * AT_HD + c], dq[c]);
    }
    for (int c = 0; c < hd; ++c) drows[(size_t)i * 3 * d + h * hd + c] = dq[c] * scale;
  }
  __syncthreads();  // K and V have been read; D and lse are in LDS
  load_head(sA, rows, 3 * d, h * hd, L, hd);                            // Q
  load_head(sB, dout + (size_t)b * L * d, d, h * hd, L, hd);            // dO
  __syncthreads();
  for (int j = threadIdx.x; j < L; j += 256) {
    float k[AT_HD], v[AT_HD], dk[AT_HD], dv[AT_HD];
#pragma unroll
    for (int c = 0; c < AT_HD; ++c) {
      k[c] = c < hd ? rows[(size_t)j * 3 * d + d + h * hd + c] : 0.f;
      v[c] = c < hd ? rows[(size_t)j * 3 * d + 2 * d + h * hd + c] : 0.f;
      dk[c] = dv[c] = 0.f;
    }
    for (int i = 0; i < L; ++i) {
      const float p = expf(dot8(sA + i * AT_HD, k) * scale - sL[i]);
      const float dS = p * (dot8(sB + i * AT_HD, v) - sD[i]);
#pragma unroll
      for (int c = 0; c < AT_HD; ++c) dv[c] = fmaf(p, sB[i * AT_HD + c], dv[c]), dk[c] = fmaf(dS, sA[i * AT_HD + c], dk[c]);
    }
    for (int c = 0; c < hd; ++c) {
      drows[(size_t)j * 3 * d + d + h * hd + c] = dk[c] * scale;
      drows[(size_t)j * 3 * d + 2 * d + h * hd + c] = dv[c];
    }
  }
}

}  // namespace ffd

static int attn_args_ok(int B, int L, int H, int hd) {
  if (B < 1 || L < 1 || H < 1 || hd < 1) return FFD_ERR_INVALID;
  if (hd > AT_HD || L > AT_MAX_L || (double)B * H > 2147483647.0 || (double)B * L * 3 * H * hd >= 2147483648.0)
    return FFD_ERR_UNSUPPORTED;
  return FFD_OK;
}

extern "C" {

int ffd_sm_draw_times_at(float* t_out, const int64_t* index, int B, double eps, double T, uint64_t seed,
                         uint64_t sample_offset, void* stream) {
  if (!t_out || !index || B < 1 || !(eps < T)) return FFD_ERR_INVALID;
  hipLaunchKernelGGL(k_sm_draw_times_at, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, t_out, index, B,
                     (float)(T - eps), (float)eps, (float)T, seed, sample_offset);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_layernorm_stats_fwd(const float* x, const float* gamma, const float* beta, float* y, float* xhat, float* rstd,
                            int M, int D, double eps, void* stream) {
  if (!x || !gamma || !beta || !y || !xhat || !rstd || M < 1 || D < 1 || !(eps >= 0.0)) return FFD_ERR_INVALID;
  if ((double)M * D >= 2147483648.0) return FFD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_ln_stats_fwd, dim3(cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, xhat, rstd, M,
                     D, (float)eps);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_layernorm_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx, float* dgamma,
                      float* dbeta, int M, int D, void* stream) {
  if (!dy || !xhat || !rstd || !gamma || !dx || !dgamma || !dbeta || M < 1 || D < 1) return FFD_ERR_INVALID;
  if ((double)M * D >= 2147483648.0 || D > 65535) return FFD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_ln_bwd, dim3(cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, dy, xhat, rstd, gamma, dx, M, D);
  hipLaunchKernelGGL(k_ln_param_grad, dim3(D), dim3(256), 0, (hipStream_t)stream, dy, xhat, dgamma, dbeta, M, D);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_attention_lse_fwd(const float* qkv, float* out, float* lse, int B, int L, int H, int hd, void* stream) {
  if (!qkv || !out || !lse) return FFD_ERR_INVALID;
  if (int rc = attn_args_ok(B, L, H, hd)) return rc;
  hipLaunchKernelGGL(k_attn_lse_fwd, dim3((unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, qkv, out, lse, L, H, hd);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int L,
                      int H, int hd, void* stream) {
  if (!qkv || !out || !dout || !lse || !dqkv || dqkv == qkv) return FFD_ERR_INVALID;
  if (int rc = attn_args_ok(B, L, H, hd)) return rc;
  hipLaunchKernelGGL(k_attn_bwd, dim3((unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, qkv, out, dout, lse, dqkv, L,
                     H, hd);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"

// ---- the transformer: ScoreModule.forward (score_models.py:79-119) keeping what the backward needs, and the backward ------
namespace ffd {

// h[b,l,:] = (h[b,l,:] + pos[l,:]) + temb[b,:]   (score_models.py:99-102)
__global__ __launch_bounds__(256) void k_add_pos_temb(float* __restrict__ h, const float* __restrict__ pos,
                                                      const float* __restrict__ temb, int L, int D, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t row = i / D;
  const int j = (int)(i - row * D), b = (int)(row / L), l = (int)(row - (size_t)b * L);
  h[i] = (h[i] + pos[(size_t)l * D + j]) + temb[(size_t)b * D + j];
}
// out[i] = sum_b dh[b][i], i < L D: the positional table's gradient (fp64, b in order)
__global__ __launch_bounds__(256) void k_sum_over_b(const float* __restrict__ dh, float* __restrict__ out, int B, int LD) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= LD) return;
  double a = 0.0;
  for (int b = 0; b < B; ++b) a += (double)dh[(size_t)b * LD + i];
  out[i] = (float)a;
}
// out[b][j] = sum_l dh[b][l][j]: the time embedding's gradient (fp64, l in order)
__global__ __launch_bounds__(256) void k_sum_over_l(const float* __restrict__ dh, float* __restrict__ out, int B, int L, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D) return;
  const int b = i / D, j = i - b * D;
  double a = 0.0;
  for (int l = 0; l < L; ++l) a += (double)dh[((size_t)b * L + l) * D + j];
  out[i] = (float)a;
}

}  // namespace ffd

namespace {

// offsets (in floats) of the transformer's workspace at batch B.  Per layer: qkv, the attention output before the
// out-projection, lse, the normalised LN1 rows and its rstd, the LN1 output, the post-ReLU hidden, the normalised LN2 rows
// and its rstd; h holds every layer's input (and the last layer's output).
struct TfWork {
  size_t xn, tb, sgb, emb, temb, h, layer, layer_size, qkv, o, lse, xh1, rs1, x1, u, xh2, rs2, y, score, dscore, dA, dB, dC, du,
      dqkv, dtemb, wg, total_bytes;
};
TfWork tf_work(const ffd_model_desc& m, int B) {
  const size_t L = m.max_len, C = m.n_channels, d = m.d_model, F = m.dim_feedforward, NL = m.num_layers, H = m.n_head, b = B;
  const size_t M = b * L;
  TfWork w;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += up4(n); return at; };
  w.xn = take(M * C), w.tb = take(b), w.sgb = take(b), w.emb = take(b * d), w.temb = take(b * d), w.h = take((NL + 1) * M * d);
  size_t q = 0;  // within a layer's block
  auto sub = [&](size_t n) { const size_t at = q; q += up4(n); return at; };
  w.qkv = sub(3 * M * d), w.o = sub(M * d), w.lse = sub(b * H * L), w.xh1 = sub(M * d), w.rs1 = sub(M), w.x1 = sub(M * d);
  w.u = sub(M * F), w.xh2 = sub(M * d), w.rs2 = sub(M);
  w.layer_size = q, w.layer = take(NL * q);
  w.y = take(M * d), w.score = take(M * C), w.dscore = take(M * C), w.dA = take(M * d), w.dB = take(M * d), w.dC = take(M * d);
  w.du = take(M * F), w.dqkv = take(3 * M * d), w.dtemb = take(b * d);
  const int Mi = (int)M, di = (int)d, Fi = (int)F, Ci = (int)C;
  size_t wg = wgrad_work_bytes(Mi, Ci, di);
  for (size_t v : {wgrad_work_bytes(Mi, di, Ci), wgrad_work_bytes(Mi, di, Fi), wgrad_work_bytes(Mi, Fi, di),
                   wgrad_work_bytes(Mi, di, di), wgrad_work_bytes(Mi, 3 * di, di), wgrad_work_bytes(B, di, di)})
    wg = std::max(wg, v);
  w.wg = take((wg + 3) / 4);
  w.total_bytes = o * sizeof(float);
  return w;
}

struct TfLayer {
  float *in_w, *in_b, *out_w, *out_b, *w1, *b1, *w2, *b2, *n1w, *n1b, *n2w, *n2b;
};
TfLayer tf_layer(ffd_train* tr, int i, bool grad) {
  const std::string p = "backbone.layers." + std::to_string(i) + ".";
  auto f = [&](const char* k) { return grad ? tr->grd(p + k) : tr->par(p + k); };
  return {f("self_attn.in_proj_weight"), f("self_attn.in_proj_bias"), f("self_attn.out_proj.weight"), f("self_attn.out_proj.bias"),
          f("linear1.weight"), f("linear1.bias"), f("linear2.weight"), f("linear2.bias"), f("norm1.weight"), f("norm1.bias"),
          f("norm2.weight"), f("norm2.bias")};
}
constexpr float TF_LN_EPS = 1e-5f;

}  // namespace

static size_t tf_work_bytes(const ffd_model_desc& m, int B) { return tf_work(m, B).total_bytes; }
static const float* tf_score(ffd_train* tr, int B) { return tr->work + tf_work(tr->desc, B).score; }

#define TRLAUNCH(...)                 \
  do {                                \
    hipLaunchKernelGGL(__VA_ARGS__);  \
    TRCHECK(hipGetLastError());       \
  } while (0)

// xn (B L, C): the network's input rows; tb (B): the per-sample times
static int tf_forward(ffd_train* tr, const float* xn, const float* tb, int B, hipStream_t s) {
  const ffd_model_desc& m = tr->desc;
  const int L = m.max_len, C = m.n_channels, d = m.d_model, F = m.dim_feedforward, NL = m.num_layers, H = m.n_head, hd = d / H;
  const int M = B * L;
  const TfWork w = tf_work(m, B);
  float* W = tr->work;
  // nn.Embedding(max_norm) renormalises the looked-up rows of the PARAMETER in place, without gradient, before the lookup
  TRCHECK(launch_renorm_rows(tr->par("pos_encoder.embedding.weight"), L, d, sqrtf((float)d), s));
  TRLAUNCH(k_time_features, dim3(cdiv(B * d, 256)), dim3(256), 0, s, tb, tr->par("time_encoder.W"), W + w.emb, B, d);
  TRCHECK(launch_dense(W + w.emb, tr->par("time_encoder.dense.weight"), tr->par("time_encoder.dense.bias"), nullptr, nullptr,
                       W + w.temb, B, d, d, 0, s));
  if (int rc = train_class_rows(tr, W + w.temb, B, s)) return rc;
  TRCHECK(launch_dense(xn, tr->par("embedder.weight"), tr->par("embedder.bias"), nullptr, nullptr, W + w.h, M, d, C, 0, s));
  const size_t Md = (size_t)M * d;
  TRLAUNCH(k_add_pos_temb, dim3((unsigned)((Md + 255) / 256)), dim3(256), 0, s, W + w.h, tr->par("pos_encoder.embedding.weight"),
           W + w.temb, L, d, Md);
  for (int i = 0; i < NL; ++i) {
    const TfLayer p = tf_layer(tr, i, false);
    float* hi = W + w.h + (size_t)i * Md;
    float* lw = W + w.layer + (size_t)i * w.layer_size;
    TRCHECK(launch_dense(hi, p.in_w, p.in_b, nullptr, nullptr, lw + w.qkv, M, 3 * d, d, 0, s));
    TRLAUNCH(k_attn_lse_fwd, dim3((unsigned)(B * H)), dim3(256), 0, s, lw + w.qkv, lw + w.o, lw + w.lse, L, H, hd);
    TRCHECK(launch_dense(lw + w.o, p.out_w, p.out_b, nullptr, hi, W + w.y, M, d, d, 0, s));
    TRLAUNCH(k_ln_stats_fwd, dim3(cdiv(M, 4)), dim3(256), 0, s, W + w.y, p.n1w, p.n1b, lw + w.x1, lw + w.xh1, lw + w.rs1, M, d,
             TF_LN_EPS);
    TRCHECK(launch_dense(lw + w.x1, p.w1, p.b1, nullptr, nullptr, lw + w.u, M, F, d, 1, s));
    TRCHECK(launch_dense(lw + w.u, p.w2, p.b2, nullptr, lw + w.x1, W + w.y, M, d, F, 0, s));
    TRLAUNCH(k_ln_stats_fwd, dim3(cdiv(M, 4)), dim3(256), 0, s, W + w.y, p.n2w, p.n2b, hi + Md, lw + w.xh2, lw + w.rs2, M, d,
             TF_LN_EPS);
  }
  TRCHECK(launch_dense(W + w.h + (size_t)NL * Md, tr->par("unembedder.weight"), tr->par("unembedder.bias"), nullptr, nullptr,
                       W + w.score, M, C, d, 0, s));
  return FFD_OK;
}

static int tf_backward(ffd_train* tr, int B, hipStream_t s) {
  const ffd_model_desc& m = tr->desc;
  const int L = m.max_len, C = m.n_channels, d = m.d_model, F = m.dim_feedforward, NL = m.num_layers, H = m.n_head, hd = d / H;
  const int M = B * L;
  const TfWork w = tf_work(m, B);
  float* W = tr->work;
  void* wg = W + w.wg;
  const size_t Md = (size_t)M * d;
  float *dh = W + w.dA, *t1 = W + w.dB, *t2 = W + w.dC;
  TRCHECK(launch_dense_wgrad(W + w.dscore, W + w.h + (size_t)NL * Md, tr->grd("unembedder.weight"), tr->grd("unembedder.bias"), M,
                             C, d, wg, s));
  TRCHECK(launch_dense_dgrad(W + w.dscore, tr->par("unembedder.weight"), nullptr, nullptr, dh, M, C, d, s));
  for (int i = NL - 1; i >= 0; --i) {
    const TfLayer p = tf_layer(tr, i, false), g = tf_layer(tr, i, true);
    const float* hi = W + w.h + (size_t)i * Md;
    float* lw = W + w.layer + (size_t)i * w.layer_size;
    // LayerNorm 2: dh -> t1 = d(x1 + ffn)
    TRLAUNCH(k_ln_bwd, dim3(cdiv(M, 4)), dim3(256), 0, s, dh, lw + w.xh2, lw + w.rs2, p.n2w, t1, M, d);
    TRLAUNCH(k_ln_param_grad, dim3(d), dim3(256), 0, s, dh, lw + w.xh2, g.n2w, g.n2b, M, d);
    // the FFN: t2 = d x1 = t1 + mask(t1 W2) W1
    TRCHECK(launch_dense_wgrad(t1, lw + w.u, g.w2, g.b2, M, d, F, wg, s));
    TRCHECK(launch_dense_dgrad(t1, p.w2, lw + w.u, nullptr, W + w.du, M, d, F, s));
    TRCHECK(launch_dense_wgrad(W + w.du, lw + w.x1, g.w1, g.b1, M, F, d, wg, s));
    TRCHECK(launch_dense_dgrad(W + w.du, p.w1, nullptr, t1, t2, M, F, d, s));
    // LayerNorm 1: t2 -> dh = d(h_i + out_proj(attention))
    TRLAUNCH(k_ln_bwd, dim3(cdiv(M, 4)), dim3(256), 0, s, t2, lw + w.xh1, lw + w.rs1, p.n1w, dh, M, d);
    TRLAUNCH(k_ln_param_grad, dim3(d), dim3(256), 0, s, t2, lw + w.xh1, g.n1w, g.n1b, M, d);
    // out-projection, attention, in-projection: t2 = d h_i = dh + dqkv Win
    TRCHECK(launch_dense_wgrad(dh, lw + w.o, g.out_w, g.out_b, M, d, d, wg, s));
    TRCHECK(launch_dense_dgrad(dh, p.out_w, nullptr, nullptr, t1, M, d, d, s));
    TRLAUNCH(k_attn_bwd, dim3((unsigned)(B * H)), dim3(256), 0, s, lw + w.qkv, lw + w.o, t1, lw + w.lse, W + w.dqkv, L, H, hd);
    TRCHECK(launch_dense_wgrad(W + w.dqkv, hi, g.in_w, g.in_b, M, 3 * d, d, wg, s));
    TRCHECK(launch_dense_dgrad(W + w.dqkv, p.in_w, nullptr, dh, t2, M, 3 * d, d, s));
    std::swap(dh, t2);
  }
  // the ends: embedder, positional table (with respect to the renormalised rows), time encoder's dense layer
  TRCHECK(launch_dense_wgrad(dh, W + w.xn, tr->grd("embedder.weight"), tr->grd("embedder.bias"), M, d, C, wg, s));
  TRLAUNCH(k_sum_over_b, dim3(cdiv(L * d, 256)), dim3(256), 0, s, dh, tr->grd("pos_encoder.embedding.weight"), B, L * d);
  TRLAUNCH(k_sum_over_l, dim3(cdiv(B * d, 256)), dim3(256), 0, s, dh, W + w.dtemb, B, L, d);
  TRCHECK(launch_dense_wgrad(W + w.dtemb, W + w.emb, tr->grd("time_encoder.dense.weight"), tr->grd("time_encoder.dense.bias"), B, d,
                             d, wg, s));
  return train_class_grad(tr, W + w.dtemb, B, s);
}

// tf_backward for the input alone: no wgrad, no LayerNorm parameter gradient, no sums over the batch or the length; one
// more dgrad through embedder.weight at the end
static int tf_input_vjp(ffd_train* tr, const float* v, float* dx, int B, hipStream_t s) {
  const ffd_model_desc& m = tr->desc;
  const int L = m.max_len, C = m.n_channels, d = m.d_model, F = m.dim_feedforward, NL = m.num_layers, H = m.n_head, hd = d / H;
  const int M = B * L;
  const TfWork w = tf_work(m, B);
  float* W = tr->work;
  float *dh = W + w.dA, *t1 = W + w.dB, *t2 = W + w.dC;
  TRCHECK(launch_dense_dgrad(v, tr->par("unembedder.weight"), nullptr, nullptr, dh, M, C, d, s));
  for (int i = NL - 1; i >= 0; --i) {
    const TfLayer p = tf_layer(tr, i, false);
    float* lw = W + w.layer + (size_t)i * w.layer_size;
    TRLAUNCH(k_ln_bwd, dim3(cdiv(M, 4)), dim3(256), 0, s, dh, lw + w.xh2, lw + w.rs2, p.n2w, t1, M, d);
    TRCHECK(launch_dense_dgrad(t1, p.w2, lw + w.u, nullptr, W + w.du, M, d, F, s));
    TRCHECK(launch_dense_dgrad(W + w.du, p.w1, nullptr, t1, t2, M, F, d, s));
    TRLAUNCH(k_ln_bwd, dim3(cdiv(M, 4)), dim3(256), 0, s, t2, lw + w.xh1, lw + w.rs1, p.n1w, dh, M, d);
    TRCHECK(launch_dense_dgrad(dh, p.out_w, nullptr, nullptr, t1, M, d, d, s));
    TRLAUNCH(k_attn_bwd, dim3((unsigned)(B * H)), dim3(256), 0, s, lw + w.qkv, lw + w.o, t1, lw + w.lse, W + w.dqkv, L, H, hd);
    TRCHECK(launch_dense_dgrad(W + w.dqkv, p.in_w, nullptr, dh, t2, M, 3 * d, d, s));
    std::swap(dh, t2);
  }
  TRCHECK(launch_dense_dgrad(dh, tr->par("embedder.weight"), nullptr, nullptr, dx, M, d, C, s));
  return FFD_OK;
}

static int tf_loss_grad(ffd_train* tr, const float* x0, const int64_t* index, const float* timesteps, const float* mean_coeff,
                        const float* sigma, const float* z, uint64_t seed, uint64_t sample_offset, int lw,
                        double* per_sample_out, int B, hipStream_t s) {
  const ffd_model_desc& m = tr->desc;
  const TfWork w = tf_work(m, B);
  float* W = tr->work;
  TRLAUNCH(k_train_perturb, dim3((unsigned)B), dim3(256), 0, s, x0, W + w.xn, timesteps, mean_coeff, sigma, tr->G_dev, z, seed,
           sample_offset, index, W + w.tb, W + w.sgb, (unsigned)m.max_len, (unsigned)m.n_channels);
  if (int rc = tf_forward(tr, W + w.xn, W + w.tb, B, s)) return rc;
  TRCHECK(launch_sm_loss_grad(W + w.score, W + w.sgb, tr->G_dev, z, seed, sample_offset, index, lw, per_sample_out,
                              W + w.dscore, B, m.max_len, m.n_channels, s));
  return tf_backward(tr, B, s);
}
