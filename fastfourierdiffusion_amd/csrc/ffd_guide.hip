// Reconstruction guidance (include/ffd.h ffd_guide_seed, ffd_guide_combine, ffd_host_guide_coef): the operators around
// the score model's input VJP in a guided step.
//   seed     x0hat = (x + c s) / alpha;  r = mask (x0hat - obs) on the time axis;  loss = 1/2 sum r^2;
//            u = d loss / d x0hat;  v = c u  (the VJP's cotangent)
//   combine  s~ = s - lambda (u + J^T v) / alpha
// k_guide_seed_time   one workgroup per sample, pointwise.  The frequency-domain seed needs both transforms and lives
//                     next to k_cond_project (ffd_fft.hip: k_guide_seed).
// k_guide_combine     pointwise, one float4 per thread where the pointers allow it.
// Every product / sum its own fp32 rounding; the loss is a fixed-order fp64 sum: bit-identical from run to run.
#include <math.h>

#include "ffd_internal.h"

namespace ffd {

namespace {

__global__ __launch_bounds__(256) void k_guide_seed_time(GuideArgs a, int L, int C) {
  __shared__ double red[256];
  const int b = blockIdx.x, per = L * C;
  const size_t sx = (size_t)b * per, so = a.obs_batch == 1 ? (size_t)0 : sx;
  double part = 0.0;
  for (int i = threadIdx.x; i < per; i += blockDim.x) {
    const size_t ix = sx + i;
    const float c = guide_c(a, i / C);
    const float xh = guide_x0hat(a, ix, c);
    if (a.x0hat) a.x0hat[ix] = xh;
    const float m = a.mask[so + i];
    const float r = __fmul_rn(m, __fsub_rn(xh, a.obs[so + i]));
    part += (double)r * (double)r;
    const float u = __fmul_rn(m, r);
    a.u[ix] = u;
    a.v[ix] = __fmul_rn(c, u);
  }
  const double total = block_sum(part, red);
  if (a.loss && threadIdx.x == 0) a.loss[b] = 0.5 * total;
}

template <bool VEC>
__global__ void k_guide_combine(const float* __restrict__ score, const float* __restrict__ u, const float* __restrict__ jtv,
                                float alpha, float coef, float* __restrict__ out, size_t n) {
  auto one = [&](float s, float uu, float j) {
    return __fsub_rn(s, __fmul_rn(coef, __fdiv_rn(__fadd_rn(uu, j), alpha)));
  };
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    if (i >= n / 4) return;
    const float4 s = reinterpret_cast<const float4*>(score)[i], uu = reinterpret_cast<const float4*>(u)[i],
                 j = reinterpret_cast<const float4*>(jtv)[i];
    reinterpret_cast<float4*>(out)[i] = make_float4(one(s.x, uu.x, j.x), one(s.y, uu.y, j.y), one(s.z, uu.z, j.z),
                                                    one(s.w, uu.w, j.w));
  } else if (i < n) {
    out[i] = one(score[i], u[i], jtv[i]);
  }
}

}  // namespace

static bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

int guide_coef(int sde, double a, double b, double t, double scale, double obs_var, double rho, double coef[3]) {
  if (!finite_nonneg(t) || !finite_nonneg(scale) || !finite_nonneg(obs_var) || !finite_nonneg(rho)) return FFD_ERR_INVALID;
  double alpha = 1.0, sigma2;
  if (sde == FFD_SDE_VP) {
    const double lmc = -0.25 * t * t * (b - a) - 0.5 * t * a;
    alpha = exp(lmc);
    sigma2 = -expm1(2.0 * lmc);
  } else {
    const double sg = a * pow(b / a, t);
    sigma2 = sg * sg;
  }
  const double den = obs_var + rho * sigma2 / (alpha * alpha + sigma2);
  if (!(den > 0.0) || !std::isfinite(den)) return FFD_ERR_INVALID;
  coef[0] = alpha, coef[1] = sigma2, coef[2] = scale / den;
  return FFD_OK;
}

hipError_t launch_guide_seed_time(const GuideArgs& a, int B, int L, int C, hipStream_t s) {
  hipLaunchKernelGGL(k_guide_seed_time, dim3((unsigned)B), dim3(256), 0, s, a, L, C);
  return hipGetLastError();
}

hipError_t launch_guide_combine(const float* score, const float* u, const float* jtv, float alpha, float coef, float* out,
                                size_t n, hipStream_t s) {
  if (n % 4 == 0 && ptr16(score) && ptr16(u) && ptr16(jtv) && ptr16(out))
    hipLaunchKernelGGL(k_guide_combine<true>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, score, u, jtv, alpha,
                       coef, out, n);
  else
    hipLaunchKernelGGL(k_guide_combine<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, score, u, jtv, alpha, coef,
                       out, n);
  return hipGetLastError();
}

}  // namespace ffd

// ---- C ABI (include/ffd.h) ----
using namespace ffd;

extern "C" {

int ffd_host_guide_coef(const ffd_sde_desc* sde, double t, double scale, double obs_var, double rho, double coef_out[3]) {
  if (!sde || !coef_out) return FFD_ERR_INVALID;
  if (!finite_nonneg(t) || !finite_nonneg(scale) || !finite_nonneg(obs_var) || !finite_nonneg(rho)) return FFD_ERR_INVALID;
  if (sde->sde != FFD_SDE_VP && sde->sde != FFD_SDE_VE) return FFD_ERR_UNSUPPORTED;
  return guide_coef(sde->sde, sde->a, sde->b, t, scale, obs_var, rho, coef_out);
}

int ffd_guide_seed(const ffd_sde_desc* sde, const float* x, const float* score, const float* obs, const float* mask,
                   const float* std, const float* G, double t, int obs_batch, int domain, int B, int L, int C,
                   float* u_out, float* v_out, double* loss_out, float* x0hat_out, void* stream) {
  if (!sde || !x || !score || !obs || !mask || !G || !u_out || !v_out || B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  if (obs_batch != 1 && obs_batch != B) return FFD_ERR_INVALID;
  if (domain != FFD_COND_FREQUENCY && domain != FFD_COND_TIME) return FFD_ERR_INVALID;
  if (domain == FFD_COND_TIME && std) return FFD_ERR_INVALID;
  if (!std::isfinite(t) || t < 0.0) return FFD_ERR_INVALID;
  const float* outs[3] = {u_out, v_out, x0hat_out};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    for (const float* in : {x, score, obs, mask, std, G})
      if (outs[i] == in) return FFD_ERR_INVALID;
    for (int j = 0; j < i; ++j)
      if (outs[i] == outs[j]) return FFD_ERR_INVALID;
  }
  if (sde->sde != FFD_SDE_VP && sde->sde != FFD_SDE_VE) return FFD_ERR_UNSUPPORTED;
  if (domain == FFD_COND_FREQUENCY && !cond_len_supported(L)) return FFD_ERR_UNSUPPORTED;
  double c[3];
  if (guide_coef(sde->sde, sde->a, sde->b, t, 0.0, 1.0, 0.0, c)) return FFD_ERR_INVALID;
  const GuideArgs a{x, score, obs, mask, std, G, u_out, v_out, x0hat_out, loss_out, (float)c[0], (float)c[1], obs_batch};
  const hipError_t e = domain == FFD_COND_TIME ? launch_guide_seed_time(a, B, L, C, (hipStream_t)stream)
                                               : launch_guide_seed_freq(a, B, L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : (e == hipErrorInvalidValue ? FFD_ERR_UNSUPPORTED : FFD_ERR_HIP);
}

int ffd_guide_combine(const float* score, const float* u, const float* jtv, float alpha, float coef, float* score_out,
                      size_t n, void* stream) {
  if (!score || !u || !jtv || !score_out || n < 1) return FFD_ERR_INVALID;
  if (!std::isfinite(alpha) || alpha == 0.0f || !std::isfinite(coef)) return FFD_ERR_INVALID;
  return launch_guide_combine(score, u, jtv, alpha, coef, score_out, n, (hipStream_t)stream) == hipSuccess ? FFD_OK
                                                                                                           : FFD_ERR_HIP;
}

}  // extern "C"
