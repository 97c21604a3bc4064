// Langevin corrector of predictor-corrector sampling (Song et al. 2021, Algorithms 4 / 5), gfx950.  The definition and
// the operation order are in include/ffd.h (ffd_langevin_step).
//   u = G_l^2 s,  w = G_l z,  n_u[b] = ||u[b]||,  n_w[b] = ||w[b]||,  eps[b] = 2 alpha (snr n_w / n_u)^2,
//   x <- x + eps[b] u + sqrt(2 eps[b]) w
// The step size needs two sample-wide norms BEFORE any element moves, so one corrector step is three stages:
//   1. k_lv_rowsq    rowsq[row] = (sum_c u^2, sum_c w^2): fp32 squares summed in fp64, c ascending
//   2. k_lv_norms    per sample a fixed-order fp64 tree over its L row partials -> n_u, n_w (and eps, sample norm)
//      k_lv_eps_batch  (batch norm only) a fixed-order mean over b -> eps
//   3. k_step<OpLangevin>  the update; on the Philox path it REGENERATES stage 1's draw (the ffd_loss.hip precedent): the
//      draw of global element g is slot g & 3 of Philox block g >> 2 whichever kernel asks, so no z buffer exists
// No atomics anywhere: the order of every sum is fixed by the element index (row l, then channel c), not by the
// thread layout, the batch size or the sample's place in the batch.
#include <math.h>

#include "ffd_step.h"

namespace ffd {

// the two fp32 squares of one element, each product its own rounding
__device__ __forceinline__ void lv_terms(float sc, float zz, float Gl, float g2, double& su, double& sw) {
  const float u = __fmul_rn(g2, sc);
  const float w = __fmul_rn(Gl, zz);
  su += (double)__fmul_rn(u, u);
  sw += (double)__fmul_rn(w, w);
}

// Stage 1: one thread per row of (B L).  VEC: C % 4 == 0, 16-byte aligned score / z and elem_offset % 4 == 0: the
// row is C / 4 float4 (each one Philox block).
template <bool VEC>
__global__ __launch_bounds__(256) void k_lv_rowsq(const float* __restrict__ score, const float* __restrict__ z,
                                                  const float* __restrict__ G, uint64_t seed, uint64_t elem_offset,
                                                  uint32_t tag, double2* __restrict__ rowsq, size_t M, int L, int C) {
  for (size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x; row < M; row += (size_t)gridDim.x * blockDim.x) {
    const float Gl = G[row % (size_t)L];
    const float g2 = __fmul_rn(Gl, Gl);
    const size_t r0 = row * (size_t)C;
    double su = 0.0, sw = 0.0;
    for (int c0 = 0; c0 < C; c0 += 4) {
      const size_t i0 = r0 + c0;
      float zz[4];
      if (VEC) {
        const float4 sc = *reinterpret_cast<const float4*>(score + i0);
        if (z) {
          const float4 zv = *reinterpret_cast<const float4*>(z + i0);
          zz[0] = zv.x, zz[1] = zv.y, zz[2] = zv.z, zz[3] = zv.w;
        } else {
          normal4((elem_offset + i0) >> 2, seed, tag, zz);
        }
        lv_terms(sc.x, zz[0], Gl, g2, su, sw);
        lv_terms(sc.y, zz[1], Gl, g2, su, sw);
        lv_terms(sc.z, zz[2], Gl, g2, su, sw);
        lv_terms(sc.w, zz[3], Gl, g2, su, sw);
      } else {
        const int n = min(4, C - c0);
        load_normals(z, i0, n, seed, elem_offset, tag, zz);
        for (int j = 0; j < n; ++j) lv_terms(score[i0 + j], zz[j], Gl, g2, su, sw);
      }
    }
    rowsq[row] = double2{su, sw};
  }
}

// eps = 2 alpha (snr n_w / n_u)^2 in fp64, rounded once to fp32; se = sqrt(2 eps) of the ROUNDED eps.  n_u == 0
// (or a non-finite ratio): eps = 0, the sample stays as it is.
__device__ __forceinline__ void lv_step_size(double nu, double nw, double snr, double alpha, float& eps, float& se) {
  eps = 0.f;
  if (nu > 0.0) {
    const double r = (snr * nw) / nu;
    const double e = (2.0 * alpha) * (r * r);
    if (e == e && e <= 3.0e38) eps = (float)e;
  }
  se = (float)sqrt(2.0 * (double)eps);
}

// Stage 2: one workgroup per sample.  Thread k adds rows k, k + 256, ... of the sample in that order, then the 256
// partials go through block_sum's fixed tree: the order depends on L alone.  SAMPLE: eps[b] follows at once.
template <bool SAMPLE>
__global__ __launch_bounds__(256) void k_lv_norms(const double2* __restrict__ rowsq, double2* __restrict__ nrm,
                                                  double snr, double alpha, float* __restrict__ eps,
                                                  float* __restrict__ se, float* __restrict__ eps_out, int L) {
  __shared__ double red[256];
  const size_t b = blockIdx.x;
  double su = 0.0, sw = 0.0;
  for (int l = threadIdx.x; l < L; l += 256) {
    const double2 v = rowsq[b * (size_t)L + l];
    su += v.x, sw += v.y;
  }
  su = block_sum(su, red);
  sw = block_sum(sw, red);
  if (threadIdx.x != 0) return;
  const double nu = sqrt(su), nw = sqrt(sw);
  nrm[b] = double2{nu, nw};
  if (SAMPLE) {
    float e, s;
    lv_step_size(nu, nw, snr, alpha, e, s);
    eps[b] = e, se[b] = s;
    if (eps_out) eps_out[b] = e;
  }
}

// Stage 2, batch norm: one workgroup.  mean_b in fp64 (thread k adds samples k, k + 256, ..., then block_sum's tree;
// the sum is divided by B), one eps for the whole batch.
__global__ __launch_bounds__(256) void k_lv_eps_batch(const double2* __restrict__ nrm, double snr, double alpha,
                                                      float* __restrict__ eps, float* __restrict__ se,
                                                      float* __restrict__ eps_out, int B) {
  __shared__ double red[256];
  double su = 0.0, sw = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) su += nrm[b].x, sw += nrm[b].y;
  su = block_sum(su, red);
  sw = block_sum(sw, red);
  float e, s;
  lv_step_size(su / (double)B, sw / (double)B, snr, alpha, e, s);
  for (int b = threadIdx.x; b < B; b += 256) {
    eps[b] = e, se[b] = s;
    if (eps_out) eps_out[b] = e;
  }
}

// x + eps u + se w, every product / sum its own fp32 rounding
__device__ __forceinline__ float lv_update(float xi, float sc, float zz, float Gl, float g2, float e, float s) {
  const float u = __fmul_rn(g2, sc);
  const float w = __fmul_rn(Gl, zz);
  return __fadd_rn(__fadd_rn(xi, __fmul_rn(e, u)), __fmul_rn(s, w));
}

// Stage 3: the op of k_step_v4 / k_step (ffd_step.h), the only one with per-sample parameters.  A sample with
// eps == 0 is not touched.
struct OpLangevin {
  static constexpr bool DRAWS = true, SAMPLE = true;
  float* x;
  const float* score;
  const float *eps, *se;
  Draws d;
  static constexpr int NIN = 2;  // x, score
  bool aligned() const { return ptr16(x) && ptr16(score); }
  __device__ bool skip(size_t b) const { return eps[b] == 0.f; }
  template <int W>
  __device__ void load(size_t i, float (&in)[NIN][W]) const {
    ld<W>(x, i, in[0]), ld<W>(score, i, in[1]);
  }
  template <int W>
  __device__ void update(size_t i, float (&in)[NIN][W], float Gl, const float (&zz)[W], size_t b) const {
    const float e = eps[b], s = se[b], g2 = __fmul_rn(Gl, Gl);
#pragma unroll
    for (int j = 0; j < W; ++j) in[0][j] = lv_update(in[0][j], in[1][j], zz[j], Gl, g2, e, s);
    st<W>(x, i, in[0]);
  }
};

size_t langevin_work_bytes(int B, int L) {
  return sizeof(double2) * (size_t)B * L + sizeof(double2) * (size_t)B + 2 * sizeof(float) * (size_t)B;
}

hipError_t launch_langevin(float* x, const float* score, const float* z, const float* G, double alpha, double snr,
                           int norm, uint64_t seed, uint64_t elem_offset, uint32_t tag, int B, int L, int C,
                           float* eps_out, void* work, hipStream_t s) {
  if (reinterpret_cast<uintptr_t>(work) & 15) return hipErrorInvalidValue;
  const size_t M = (size_t)B * L;
  double2* rowsq = static_cast<double2*>(work);
  double2* nrm = rowsq + M;
  float* eps = reinterpret_cast<float*>(nrm + B);
  float* se = eps + B;
  const bool vec = C % 4 == 0 && ptr16(x) && ptr16(score) && ptr16(z) && elem_offset % 4 == 0;
  size_t blocks = (M + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (vec)
    hipLaunchKernelGGL(k_lv_rowsq<true>, dim3((unsigned)blocks), dim3(256), 0, s, score, z, G, seed, elem_offset, tag, rowsq,
                       M, L, C);
  else
    hipLaunchKernelGGL(k_lv_rowsq<false>, dim3((unsigned)blocks), dim3(256), 0, s, score, z, G, seed, elem_offset, tag, rowsq,
                       M, L, C);
  if (norm == FFD_LANGEVIN_NORM_SAMPLE) {
    hipLaunchKernelGGL(k_lv_norms<true>, dim3((unsigned)B), dim3(256), 0, s, rowsq, nrm, snr, alpha, eps, se, eps_out, L);
  } else {
    hipLaunchKernelGGL(k_lv_norms<false>, dim3((unsigned)B), dim3(256), 0, s, rowsq, nrm, snr, alpha, eps, se, eps_out, L);
    hipLaunchKernelGGL(k_lv_eps_batch, dim3(1), dim3(256), 0, s, nrm, snr, alpha, eps, se, eps_out, B);
  }
  return launch_step(OpLangevin{x, score, eps, se, Draws{z, seed, elem_offset, tag}}, G, B, L, C, s);
}

double langevin_alpha(int sde, double a, double b, double t, float step_size) {
  if (sde != FFD_SDE_VP) return 1.0;
  const double alpha = 1.0 - (a + t * (b - a)) * (double)step_size;  // score_sde's 1 - beta_i on this grid
  return alpha > 0.0 ? alpha : 0.0;
}

}  // namespace ffd

using namespace ffd;

extern "C" {

size_t ffd_langevin_work_bytes(int B, int L) { return (B < 1 || L < 1) ? 0 : langevin_work_bytes(B, L); }

int ffd_langevin_step(const ffd_sde_desc* sde, float* x, const float* score, const float* G, double t, float step_size,
                      float snr, int norm, const float* z, uint64_t seed, uint64_t sample_offset, uint32_t tag, int B, int L,
                      int C, float* eps_out, void* work, void* stream) {
  if (!sde || !x || !score || !G || !work || B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  if (!(snr > 0.f) || !(step_size > 0.f) || x == score) return FFD_ERR_INVALID;
  if (norm != FFD_LANGEVIN_NORM_BATCH && norm != FFD_LANGEVIN_NORM_SAMPLE) return FFD_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(work) & 15) return FFD_ERR_INVALID;
  if (sde->sde != FFD_SDE_VP && sde->sde != FFD_SDE_VE) return FFD_ERR_UNSUPPORTED;
  hipError_t e = launch_langevin(x, score, z, G, langevin_alpha(sde->sde, sde->a, sde->b, t, step_size), (double)snr, norm,
                                 seed, sample_offset * (uint64_t)L * C, tag, B, L, C, eps_out, work, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"
