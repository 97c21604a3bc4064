// Denoising score-matching loss on the device (fdiff.utils.losses.get_sde_loss_fn, losses.py:54-125; the forward
// perturbation is SDE.marginal_prob + SDE.add_noise, sde.py:66-77,106-123,187-210).
//
//   k_sm_draw_times   t = u (T - eps) + eps, u from Philox4x32-10 by global sample index            (losses.py:60-63)
//   k_sm_perturb(_v4) x_noisy = mean_coeff[b] x0 + (sigma[b] G[l]) z: 12 B per element, 16 B with injected z
//   k_sm_loss         one workgroup per sample: r = score + z / std, fp32 terms w r^2 or (std r)^2, fp64 partials and a
//                     fixed-order LDS tree; with z == nullptr it regenerates the draws the perturbation made
//
// The reference forms std (B, L) = sigma[b] G[l] and multiplies by dense diag(std), diag(1 / std) matrices; the kernels
// evaluate the same products element-wise, each rounded like the reference's separate torch op (no FMA contraction).
// mean_coeff and sigma are inputs: VP's sqrt(1 - exp(2 lmc)) is too ill-conditioned to recompute here (include/ffd.h).
// The entry points that need no context follow the kernels; ffd_sm_eval_batch is in ffd_api.hip.
#include "ffd_internal.h"

namespace ffd {

__global__ __launch_bounds__(256) void k_sm_draw_times(float* __restrict__ t, int B, float span, float eps, float T,
                                                       uint64_t seed, uint64_t sample_offset) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const uint64_t g = sample_offset + (uint64_t)i;  // slot g & 3 of block g >> 2, as the element draws are counted
  const U4 c = {(uint32_t)(g >> 2), (uint32_t)(g >> 34), SM_TAG_TIMES, 0x46464446u};
  const U4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int sl = (int)(g & 3);
  const uint32_t w = sl == 0 ? r.x : sl == 1 ? r.y : sl == 2 ? r.z : r.w;
  const float u = (float)(w >> 8) * (1.0f / 16777216.0f);  // [0, 1), like torch.rand
  t[i] = fminf(__fadd_rn(__fmul_rn(u, span), eps), T);
}

__device__ __forceinline__ float perturb_value(float mc, float x, float sd, float z) {
  return __fadd_rn(__fmul_rn(mc, x), __fmul_rn(sd, z));  // mean + noise (sde.py:76)
}

// (L C) % 4 == 0 and 16-byte aligned buffers: a float4 never crosses a sample, and the draws of an aligned quad are one
// Philox block.  nq = quads per sample.  The quad's elements share G[l] unless it crosses a row (C % 4 != 0).
__global__ __launch_bounds__(256) void k_sm_perturb_v4(const float* __restrict__ x0, float* __restrict__ xn,
                                                       const float* __restrict__ mc, const float* __restrict__ sigma,
                                                       const float* __restrict__ G, const float* __restrict__ z,
                                                       uint64_t seed, uint64_t elem_offset, size_t nvec, unsigned nq,
                                                       unsigned C) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    const size_t b = v / nq;
    const unsigned r = (unsigned)(v - b * nq) << 2;  // first element of the quad within its sample
    const unsigned l0 = r / C, c0 = r - l0 * C;
    const float4 x = reinterpret_cast<const float4*>(x0)[v];
    float zz[4];
    if (z) {
      const float4 zv = reinterpret_cast<const float4*>(z)[v];
      zz[0] = zv.x, zz[1] = zv.y, zz[2] = zv.z, zz[3] = zv.w;
    } else {
      normal4((elem_offset >> 2) + v, seed, SM_TAG_NOISE, zz);  // elem_offset is a multiple of L C
    }
    const float m = mc[b], sg = sigma[b];
    float sd[4];
    if (c0 + 3 < C) {
      sd[0] = sd[1] = sd[2] = sd[3] = __fmul_rn(sg, G[l0]);
    } else {
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) sd[j] = __fmul_rn(sg, G[l0 + (c0 + j) / C]);
    }
    reinterpret_cast<float4*>(xn)[v] = float4{perturb_value(m, x.x, sd[0], zz[0]), perturb_value(m, x.y, sd[1], zz[1]),
                                              perturb_value(m, x.z, sd[2], zz[2]), perturb_value(m, x.w, sd[3], zz[3])};
  }
}

// any L C and alignment: four consecutive elements per thread, each with its own sample and row
__global__ __launch_bounds__(256) void k_sm_perturb(const float* __restrict__ x0, float* __restrict__ xn,
                                                    const float* __restrict__ mc, const float* __restrict__ sigma,
                                                    const float* __restrict__ G, const float* __restrict__ z,
                                                    uint64_t seed, uint64_t elem_offset, size_t total, unsigned n,
                                                    unsigned C) {
  const size_t nvec = (total + 3) / 4;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    const size_t i0 = v * 4;
    const int cnt = (int)((total - i0) < 4 ? (total - i0) : 4);
    float zz[4];
    load_normals(z, i0, cnt, seed, elem_offset, SM_TAG_NOISE, zz);
    for (int j = 0; j < cnt; ++j) {
      const size_t i = i0 + j;
      const size_t b = i / n;
      const unsigned l = (unsigned)(i - b * n) / C;
      xn[i] = perturb_value(mc[b], x0[i], __fmul_rn(sigma[b], G[l]), zz[j]);
    }
  }
}

hipError_t launch_sm_perturb(const float* x0, float* x_noisy, const float* mean_coeff, const float* sigma, const float* G,
                             const float* z, uint64_t seed, uint64_t sample_offset, int B, int L, int C, hipStream_t s) {
  const unsigned n = (unsigned)L * (unsigned)C;
  const size_t total = (size_t)B * n;
  size_t blocks = ((total + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const uint64_t elem_offset = sample_offset * (uint64_t)n;
  if (n % 4 == 0 && ptr16(x0) && ptr16(x_noisy) && ptr16(z))
    hipLaunchKernelGGL(k_sm_perturb_v4, dim3((unsigned)blocks), dim3(256), 0, s, x0, x_noisy, mean_coeff, sigma, G, z, seed,
                       elem_offset, total / 4, n / 4, (unsigned)C);
  else
    hipLaunchKernelGGL(k_sm_perturb, dim3((unsigned)blocks), dim3(256), 0, s, x0, x_noisy, mean_coeff, sigma, G, z, seed,
                       elem_offset, total, n, (unsigned)C);
  return hipGetLastError();
}

// One term of the loss (losses.py:68-80,100-102,115-121): target = (1 / std) z, r = score + target, then r^2 (the
// weighting factor is applied to the sum) or (std r)^2.
template <bool LW>
__device__ __forceinline__ float loss_term(float sc, float zv, float sd) {
  const float r = __fadd_rn(sc, __fmul_rn(__fdiv_rn(1.0f, sd), zv));
  const float q = LW ? __fmul_rn(sd, r) : r;
  return __fmul_rn(q, q);
}

// One workgroup per sample.  The sample's elements are walked as the aligned quads of the GLOBAL element index
// g = (sample_offset + b) L C + r (thread t takes quads t, t + 256, ... of the sample's range, the elements of a quad in
// order): a quad is one Philox block, and the order of the sum depends on the global sample index only, not on how a
// batch is cut into calls.  VEC: L C % 4 == 0 and aligned buffers, so the quads are float4 of score (and z).
template <bool VEC, bool LW>
__global__ __launch_bounds__(256) void k_sm_loss(const float* __restrict__ score, const float* __restrict__ sigma,
                                                 const float* __restrict__ G, const float* __restrict__ z, uint64_t seed,
                                                 uint64_t sample_offset, int reduce_mean, double* __restrict__ out,
                                                 unsigned L, unsigned C) {
  __shared__ double red[256];
  const unsigned b = blockIdx.x, n = L * C;
  const float sg = sigma[b];
  const uint64_t g0 = (sample_offset + b) * (uint64_t)n, g1 = g0 + n;
  const size_t base = (size_t)b * n;
  const uint64_t q_first = g0 >> 2, q_last = (g1 - 1) >> 2;
  double acc = 0.0;
  for (uint64_t q = q_first + threadIdx.x; q <= q_last; q += 256) {
    float zz[4];
    if (!z) normal4(q, seed, SM_TAG_NOISE, zz);
    if (VEC) {  // g0 % 4 == 0: the whole quad belongs to the sample
      const unsigned r = (unsigned)(q - q_first) << 2;
      const unsigned l0 = r / C, c0 = r - l0 * C;
      const float4 sc = *reinterpret_cast<const float4*>(score + base + r);
      if (z) {
        const float4 zv = *reinterpret_cast<const float4*>(z + base + r);
        zz[0] = zv.x, zz[1] = zv.y, zz[2] = zv.z, zz[3] = zv.w;
      }
      float sd[4];
      if (c0 + 3 < C) {
        sd[0] = sd[1] = sd[2] = sd[3] = __fmul_rn(sg, G[l0]);
      } else {
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) sd[j] = __fmul_rn(sg, G[l0 + (c0 + j) / C]);
      }
      acc += (double)loss_term<LW>(sc.x, zz[0], sd[0]);
      acc += (double)loss_term<LW>(sc.y, zz[1], sd[1]);
      acc += (double)loss_term<LW>(sc.z, zz[2], sd[2]);
      acc += (double)loss_term<LW>(sc.w, zz[3], sd[3]);
    } else {
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) {
        const uint64_t g = (q << 2) + j;
        if (g < g0 || g >= g1) continue;
        const unsigned r = (unsigned)(g - g0);
        const float zv = z ? z[base + r] : zz[j];
        acc += (double)loss_term<LW>(score[base + r], zv, __fmul_rn(sg, G[r / C]));
      }
    }
  }
  double total = block_sum(acc, red);
  if (!LW) {  // weighting_factor = 1 / sum_l (1 / std^2) (losses.py:96), summed in fp64
    double ws = 0.0;
    for (unsigned l = threadIdx.x; l < L; l += 256) {
      const double sd = (double)__fmul_rn(sg, G[l]);
      ws += 1.0 / (sd * sd);
    }
    total /= block_sum(ws, red);
  }
  if (threadIdx.x == 0) out[b] = reduce_mean ? total / (double)n : 0.5 * total;  // losses.py:33-37
}

hipError_t launch_sm_loss(const float* score, const float* sigma, const float* G, const float* z, uint64_t seed,
                          uint64_t sample_offset, int likelihood_weighting, int reduce_mean, double* out, int B, int L,
                          int C, hipStream_t s) {
  const bool vec = ((unsigned)L * (unsigned)C) % 4 == 0 && ptr16(score) && ptr16(z);
#define FFD_SM_LOSS(v, lw)                                                                                             \
  hipLaunchKernelGGL((k_sm_loss<v, lw>), dim3((unsigned)B), dim3(256), 0, s, score, sigma, G, z, seed, sample_offset,  \
                     reduce_mean, out, (unsigned)L, (unsigned)C)
  if (vec && likelihood_weighting) FFD_SM_LOSS(true, true);
  else if (vec) FFD_SM_LOSS(true, false);
  else if (likelihood_weighting) FFD_SM_LOSS(false, true);
  else FFD_SM_LOSS(false, false);
#undef FFD_SM_LOSS
  return hipGetLastError();
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): the context-free entry points of the score-matching loss ----
using namespace ffd;

extern "C" {

static int sm_check_shape(int B, int L, int C) {
  if (B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  if ((double)L * C >= 2147483648.0) return FFD_ERR_UNSUPPORTED;  // a sample's elements are indexed in 32 bits
  return FFD_OK;
}

int ffd_sm_draw_times(float* t_out, int B, double eps, double T, uint64_t seed, uint64_t sample_offset, void* stream) {
  if (!t_out || B < 1 || !(eps < T)) return FFD_ERR_INVALID;
  hipLaunchKernelGGL(k_sm_draw_times, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, t_out, B, (float)(T - eps),
                     (float)eps, (float)T, seed, sample_offset);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_sm_perturb(const float* x0, float* x_noisy, const float* mean_coeff, const float* sigma, const float* G,
                   const float* z, uint64_t seed, uint64_t sample_offset, int B, int L, int C, void* stream) {
  if (!x0 || !x_noisy || !mean_coeff || !sigma || !G || x0 == x_noisy) return FFD_ERR_INVALID;
  if (int rc = sm_check_shape(B, L, C)) return rc;
  return launch_sm_perturb(x0, x_noisy, mean_coeff, sigma, G, z, seed, sample_offset, B, L, C, (hipStream_t)stream) ==
                 hipSuccess
             ? FFD_OK
             : FFD_ERR_HIP;
}

int ffd_sm_loss(const float* score, const float* sigma, const float* G, const float* z, uint64_t seed,
                uint64_t sample_offset, int likelihood_weighting, int reduce_mean, double* per_sample_out, int B, int L,
                int C, void* stream) {
  if (!score || !sigma || !G || !per_sample_out) return FFD_ERR_INVALID;
  if (int rc = sm_check_shape(B, L, C)) return rc;
  return launch_sm_loss(score, sigma, G, z, seed, sample_offset, likelihood_weighting, reduce_mean, per_sample_out, B, L,
                        C, (hipStream_t)stream) == hipSuccess
             ? FFD_OK
             : FFD_ERR_HIP;
}

}  // extern "C"
