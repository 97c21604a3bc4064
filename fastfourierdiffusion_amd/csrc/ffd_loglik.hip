// Log-likelihoods through the probability-flow ODE (Song et al. 2021, section 4.3 / appendix D.2), gfx950.  The
// definition and the operation order are in include/ffd.h (ffd_loglik_tail).  One divergence evaluation at (x, t) is
//   1. k_ll_perturb   the stacked batch of (1 + 2 k) B rows: x, then x + h w_m, x - h w_m per probe m, w_m = G_l eps_m
//   2. (the score network at the stacked batch: the caller's forward)
//   3. k_ll_tail      one workgroup per sample: the fp64 sum of w_m (s+ - s-) over the sample, the divergence term v,
//                     the state update from block 0's score with ode_drift's rounding, and delta (or Heun's v1)
// On the Philox path the tail REGENERATES the probes the perturbation drew (the ffd_langevin.hip precedent): the
// Rademacher value of global element g under tag T is bit 31 of slot g & 3 of Philox block g >> 2, whichever kernel
// asks, so no probe buffer exists.  k_ll_prior is the log-density of ffd_prior's Gaussian.
// No atomics: every sample-wide sum has an order fixed by the element index i = l C + c (and the probe index) alone --
// thread p of the sample's workgroup adds, probe by probe, elements p, p + 256, ... in ascending order, then the 256
// partials go through block_sum's fixed tree -- so the result does not depend on B or on the sample's place.
#include <math.h>

#include "ffd_step.h"

namespace ffd {

// +1 / -1 from bit 31 of the Philox word of global element g under (seed, tag)
__device__ __forceinline__ float rademacher(uint64_t g, uint64_t seed, uint32_t tag) {
  const uint64_t g4 = g >> 2;
  const U4 r = philox4x32_10(U4{(uint32_t)g4, (uint32_t)(g4 >> 32), tag, 0x46464446u /* "FFDF" */}, (uint32_t)seed,
                             (uint32_t)(seed >> 32));
  const uint32_t slot = (uint32_t)(g & 3);
  const uint32_t w = slot == 0 ? r.x : slot == 1 ? r.y : slot == 2 ? r.z : r.w;
  return (w >> 31) ? -1.f : 1.f;
}

// probe m of element i (of the call's B L C = n): the injected slab, or the draw of global element elem_offset + i
__device__ __forceinline__ float probe_at(const LoglikProbes& pr, int m, size_t i, size_t n) {
  return pr.inject ? pr.inject[(size_t)m * n + i] : rademacher(pr.elem_offset + i, pr.seed, pr.tag0 + (uint32_t)m);
}

// stack block 0 = x, block 2 m + 1 = x + h w_m, block 2 m + 2 = x - h w_m (m = 0 .. k - 1); one element per thread and
// iteration, w = G_l eps, hw = h w, each its own fp32 rounding
__global__ __launch_bounds__(256) void k_ll_perturb(const float* __restrict__ x, float* __restrict__ stack,
                                                    const float* __restrict__ G, float h, LoglikProbes pr, size_t n, int L,
                                                    int C) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float xi = x[i], Gl = G[(i / (size_t)C) % (size_t)L];
    stack[i] = xi;
    for (int m = 0; m < pr.k; ++m) {
      const float hw = __fmul_rn(h, __fmul_rn(Gl, probe_at(pr, m, i, n)));
      stack[(size_t)(2 * m + 1) * n + i] = __fadd_rn(xi, hw);
      stack[(size_t)(2 * m + 2) * n + i] = __fsub_rn(xi, hw);
    }
  }
}

struct LoglikTail {
  float *x, *xp, *d1;
  const float *score, *G;
  LoglikProbes pr;
  SdeParams p;         // a, cs at the evaluation's time; dt = (float) of the interval's width
  double aLC, c2, den;  // v = aLC + c2 (sum / den): a(t) L C, -cs(t)^2 / 2, 2 h k
  double dt;
  double *delta, *v1, *v_out;
  size_t n;  // B L C
  int L, C;
};

// One workgroup per sample.  The reduction reads the score blocks 1 .. 2 k and the probes; the state update reads block 0
// (the score at the evaluated point) and writes x / xp / d1, none of which the reduction touches.
template <int STAGE>
__global__ __launch_bounds__(256) void k_ll_tail(LoglikTail a) {
  __shared__ double red[256];
  const size_t per = (size_t)a.L * a.C, base = (size_t)blockIdx.x * per;
  double acc = 0.0;
  for (int m = 0; m < a.pr.k; ++m) {
    const float* sp = a.score + (size_t)(2 * m + 1) * a.n + base;
    const float* sm = a.score + (size_t)(2 * m + 2) * a.n + base;
    for (size_t i = threadIdx.x; i < per; i += 256) {
      const float w = __fmul_rn(a.G[i / (size_t)a.C], probe_at(a.pr, m, base + i, a.n));
      acc += (double)__fmul_rn(w, __fsub_rn(sp[i], sm[i]));
    }
  }
  const double total = block_sum(acc, red);
  for (size_t i = threadIdx.x; i < per; i += 256) {
    const size_t e = base + i;
    const float Gl = a.G[i / (size_t)a.C];
    if (STAGE == LL_CORRECT) {  // score = the score at xp; x = what the predictor read
      const float d = ode_drift(a.xp[e], a.score[e], Gl, a.p);
      a.x[e] = __fadd_rn(a.x[e], __fmul_rn(__fmul_rn(0.5f, __fadd_rn(a.d1[e], d)), a.p.dt));
    } else {
      const float xi = a.x[e];
      const float d = ode_drift(xi, a.score[e], Gl, a.p);
      const float xn = __fadd_rn(xi, __fmul_rn(d, a.p.dt));
      if (STAGE == LL_PREDICT) a.d1[e] = d, a.xp[e] = xn;
      else a.x[e] = xn;
    }
  }
  if (threadIdx.x != 0) return;
  const size_t b = blockIdx.x;
  const double v = __dadd_rn(a.aLC, __dmul_rn(a.c2, total / a.den));
  if (a.v_out) a.v_out[b] = v;
  if (STAGE == LL_EULER) a.delta[b] = __dadd_rn(a.delta[b], __dmul_rn(a.dt, v));
  if (STAGE == LL_PREDICT) a.v1[b] = v;
  if (STAGE == LL_CORRECT) a.delta[b] = __dadd_rn(a.delta[b], __dmul_rn(0.5 * a.dt, __dadd_rn(a.v1[b], v)));
}

// log N(x; 0, (scale G_l)^2) per element: sg = scale G_l, q = x / sg, term = (-0.5 (q q)) - (float)(log sg + log(2 pi) / 2),
// each its own fp32 rounding (the logarithm in fp64, rounded once); the sample's terms are summed in fp64
__global__ __launch_bounds__(256) void k_ll_prior(const float* __restrict__ x, const float* __restrict__ G, float scale,
                                                  double* __restrict__ out, int L, int C) {
  __shared__ double red[256];
  const size_t per = (size_t)L * C, base = (size_t)blockIdx.x * per;
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < per; i += 256) {
    const float sg = __fmul_rn(scale, G[i / (size_t)C]);
    const float q = __fdiv_rn(x[base + i], sg);
    const float c = (float)(log((double)sg) + 0.91893853320467274178);
    acc += (double)__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(q, q)), c);
  }
  const double total = block_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = total;
}

double loglik_sigma(int sde, double a, double b, double t) {
  if (sde == FFD_SDE_VP) return sqrt(-expm1(2.0 * (-0.25 * t * t * (b - a) - 0.5 * t * a)));
  return a * pow(b / a, t);
}

bool loglik_shape_supported(int n_probes, int B, int L, int C) {
  return (double)(1 + 2 * (double)n_probes) * B * L * C < 2147483648.0;
}

hipError_t launch_loglik_perturb(const float* x, float* stack, const float* G, float h, LoglikProbes pr, int B, int L, int C,
                                 hipStream_t s) {
  const size_t n = (size_t)B * L * C;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_ll_perturb, dim3((unsigned)blocks), dim3(256), 0, s, x, stack, G, h, pr, n, L, C);
  return hipGetLastError();
}

hipError_t launch_loglik_tail(int stage, int sde, double a, double b, double t, double dt, float h, float* x, float* xp,
                              float* d1, const float* score, const float* G, LoglikProbes pr, double* delta, double* v1,
                              double* v_out, int B, int L, int C, hipStream_t s) {
  LoglikTail k{x, xp, d1, score, G, pr, sde_params(sde, a, b, t, (float)dt), 0.0, 0.0, 2.0 * (double)h * (double)pr.k, dt,
               delta, v1, v_out, (size_t)B * L * C, L, C};
  if (sde == FFD_SDE_VP) {
    const double beta = a + t * (b - a);
    k.aLC = (-0.5 * beta) * (double)((size_t)L * C);
    k.c2 = -0.5 * beta;
  } else {
    const double r = b / a, cs = a * sqrt(2.0 * log(r)) * pow(r, t);
    k.c2 = -0.5 * (cs * cs);
  }
  switch (stage) {
    case LL_EULER: hipLaunchKernelGGL(k_ll_tail<LL_EULER>, dim3((unsigned)B), dim3(256), 0, s, k); break;
    case LL_PREDICT: hipLaunchKernelGGL(k_ll_tail<LL_PREDICT>, dim3((unsigned)B), dim3(256), 0, s, k); break;
    case LL_CORRECT: hipLaunchKernelGGL(k_ll_tail<LL_CORRECT>, dim3((unsigned)B), dim3(256), 0, s, k); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_prior_logp(const float* x, const float* G, float scale, double* out, int B, int L, int C, hipStream_t s) {
  hipLaunchKernelGGL(k_ll_prior, dim3((unsigned)B), dim3(256), 0, s, x, G, scale, out, L, C);
  return hipGetLastError();
}

}  // namespace ffd

using namespace ffd;

namespace {

bool known_sde(const ffd_sde_desc* sde) { return sde->sde == FFD_SDE_VP || sde->sde == FFD_SDE_VE; }
bool finite_pos(double v) { return v > 0.0 && v <= 1.7e308; }

// [p, p + n floats) and [q, q + m floats) share an address
bool overlap(const void* p, size_t n, const void* q, size_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return p && q && a < b + 4 * m && b < a + 4 * n;
}

}  // namespace

extern "C" {

int ffd_host_loglik_h(const ffd_sde_desc* sde, double t, double fd_rel, float* h_out) {
  if (!sde || !h_out || !known_sde(sde) || !finite_pos(fd_rel) || !(t >= 0.0 && t <= 1.7e308)) return FFD_ERR_INVALID;
  const float h = (float)(fd_rel * loglik_sigma(sde->sde, sde->a, sde->b, t));
  if (!finite_pos((double)h)) return FFD_ERR_INVALID;
  *h_out = h;
  return FFD_OK;
}

int ffd_prior_logp(const ffd_sde_desc* sde, const float* x, const float* G, double* logp_out, int B, int L, int C,
                   void* stream) {
  if (!sde || !x || !G || !logp_out || B < 1 || L < 1 || C < 1 || !known_sde(sde)) return FFD_ERR_INVALID;
  if (!loglik_shape_supported(0, B, L, C)) return FFD_ERR_UNSUPPORTED;
  if (overlap(logp_out, 2 * (size_t)B, x, (size_t)B * L * C) || overlap(logp_out, 2 * (size_t)B, G, L)) return FFD_ERR_INVALID;
  const float scale = sde->sde == FFD_SDE_VE ? (float)sde->b : 1.f;
  if (!finite_pos((double)scale)) return FFD_ERR_INVALID;
  return launch_prior_logp(x, G, scale, logp_out, B, L, C, (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_loglik_perturb(const float* x, const float* G, float h, int n_probes, const float* probes, uint64_t seed,
                       uint64_t sample_offset, uint32_t tag0, float* stack_out, int B, int L, int C, void* stream) {
  if (!x || !G || !stack_out || B < 1 || L < 1 || C < 1 || n_probes < 1 || !finite_pos((double)h)) return FFD_ERR_INVALID;
  if (!loglik_shape_supported(n_probes, B, L, C)) return FFD_ERR_UNSUPPORTED;
  const size_t n = (size_t)B * L * C, rows = (size_t)(1 + 2 * n_probes) * n;
  if (overlap(stack_out, rows, x, n) || overlap(stack_out, rows, probes, (size_t)n_probes * n) || overlap(stack_out, rows, G, L))
    return FFD_ERR_INVALID;
  const LoglikProbes pr{probes, seed, sample_offset * (uint64_t)L * C, tag0, n_probes};
  return launch_loglik_perturb(x, stack_out, G, h, pr, B, L, C, (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_loglik_tail(const ffd_sde_desc* sde, int stage, float* x, float* x_pred, float* drift, const float* score_stack,
                    const float* G, double t, double dt, float h, int n_probes, const float* probes, uint64_t seed,
                    uint64_t sample_offset, uint32_t tag0, double* delta, double* v1, double* v_out, int B, int L, int C,
                    void* stream) {
  if (!sde || !x || !score_stack || !G || B < 1 || L < 1 || C < 1 || n_probes < 1) return FFD_ERR_INVALID;
  if (stage != FFD_LOGLIK_EULER && stage != FFD_LOGLIK_PREDICT && stage != FFD_LOGLIK_CORRECT) return FFD_ERR_INVALID;
  if (!known_sde(sde) || !finite_pos((double)h) || !finite_pos(dt) || !finite_pos((double)(float)dt)) return FFD_ERR_INVALID;
  if (!(t >= 0.0 && t <= 1.7e308)) return FFD_ERR_INVALID;
  const bool heun = stage != FFD_LOGLIK_EULER;
  if (heun && (!x_pred || !drift || !v1)) return FFD_ERR_INVALID;
  if (stage != FFD_LOGLIK_PREDICT && !delta) return FFD_ERR_INVALID;
  if (!loglik_shape_supported(n_probes, B, L, C)) return FFD_ERR_UNSUPPORTED;
  const size_t n = (size_t)B * L * C, rows = (size_t)(1 + 2 * n_probes) * n;
  // the buffers the call writes may not share an address with each other or with anything it reads
  const void* state[3] = {x, heun ? x_pred : nullptr, heun ? drift : nullptr};
  for (int i = 0; i < 3; ++i) {
    if (overlap(state[i], n, score_stack, rows) || overlap(state[i], n, probes, (size_t)n_probes * n) ||
        overlap(state[i], n, G, L))
      return FFD_ERR_INVALID;
    for (int j = i + 1; j < 3; ++j)
      if (overlap(state[i], n, state[j], n)) return FFD_ERR_INVALID;
  }
  const void* sums[3] = {stage != FFD_LOGLIK_PREDICT ? delta : nullptr, heun ? v1 : nullptr, v_out};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      if (overlap(sums[i], 2 * (size_t)B, state[j], n)) return FFD_ERR_INVALID;
    if (overlap(sums[i], 2 * (size_t)B, score_stack, rows) || overlap(sums[i], 2 * (size_t)B, probes, (size_t)n_probes * n) ||
        overlap(sums[i], 2 * (size_t)B, G, L))
      return FFD_ERR_INVALID;
    for (int j = i + 1; j < 3; ++j)
      if (overlap(sums[i], 2 * (size_t)B, sums[j], 2 * (size_t)B)) return FFD_ERR_INVALID;
  }
  const LoglikProbes pr{probes, seed, sample_offset * (uint64_t)L * C, tag0, n_probes};
  const hipError_t e = launch_loglik_tail(stage, sde->sde, sde->a, sde->b, t, dt, h, x, x_pred, drift, score_stack, G, pr,
                                          delta, v1, v_out, B, L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"
