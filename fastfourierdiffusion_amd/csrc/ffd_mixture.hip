// The closed-form score of a diffused Gaussian mixture (include/ffd.h ffd_mixture_score): the "optimal denoiser" of
//   p_0 = sum_i w_i N(mu_i, diag(v))   under   x_t = alpha(t) x_0 + sigma(t) G_l z,
//   c_lc = alpha^2 v_lc + sigma^2 G_l^2,  logit_i = log w_i - 1/2 sum_lc (x_lc - alpha mu_i,lc)^2 / c_lc,
//   r = softmax_i(logit),  d = alpha sum_i r_i mu_i - x,  score = d / c.
// An attention-shaped kernel: the rows of x are the queries, the K component means are keys and values.
//
// k_mixture_part   grid (row tiles of 16, component slices of 512).  A workgroup of four waves keeps its 16 rows of x and
//                  of 1 / c in registers (a lane owns every 16th float4 of one row), streams its slice's means through
//                  LDS in tiles of 16 components (the next tile's global loads are in flight while the current one is
//                  worked on), forms the logits on the vector pipe in DIFFERENCE form -- t = x - alpha mu in one FMA,
//                  then t (t / c) summed -- keeps an online softmax (running max and sum) per row, and accumulates
//                  sum_i p_i mu_i on the fp32 matrix cores (16x16x4: rows x components x 16 coordinates; a wave owns a
//                  quarter of the coordinates).  It leaves (max, sum, weighted sum) per (slice, row).
// k_mixture_merge  one workgroup per row: combines the slices in ascending order and forms d and the score.
// The vector-Jacobian product J^T v of the score with respect to x (ffd_mixture_score_vjp) is a second instance of
// k_mixture_part with a merge of its own (k_mixture_vjp_merge): a pass of its own, so the score's instance keeps its
// registers.
// No atomics and no order that depends on timing: bit-identical from run to run.  The tiling depends on K and L C
// alone, never on B, and a row's arithmetic does not depend on its place in a tile, so a row's result does not depend on
// the batch it came in; shared and per-sample times are one code path (t[row * t_stride]).
#include <math.h>

#include "ffd_internal.h"

namespace ffd {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int RT = MIX_ROW_TILE, KT = MIX_COMP_TILE, SL = MIX_SLICE;
static_assert(RT == 16 && KT == 16, "the MFMA fragment maps and the 16-lane row groups assume 16 x 16 tiles");
constexpr int PART_STRIDE = KT * 16 + 16;  // floats per row of the partial-sum image (+16: the two row groups of a
                                           // 32-lane read land on different banks)

struct MixArgs {
  const float *x, *t, *means, *logw, *var, *G;
  float* work;
  float* out;
  double sa, sb;
  int sde, t_stride, B, K, L, C, D;
  const float* v;  // the VJP instance's cotangent (B, L, C); unused by the score
};

// alpha and sigma^2 of the forward marginal at the fp32 grid value t, formed in double and rounded once.
// VP: sigma^2 = -expm1(2 log alpha) (nothing is lost to 1 - exp(.) at small t).
__device__ __forceinline__ void mix_coeffs(int sde, double a, double b, float tf, float& alpha, float& sigma2) {
  const double t = (double)tf;
  if (sde == FFD_SDE_VP) {
    const double la = -0.25 * t * t * (b - a) - 0.5 * t * a;
    alpha = (float)exp(la);
    sigma2 = (float)(-expm1(2.0 * la));
  } else {
    const double sg = a * exp(t * log(b / a));
    alpha = 1.0f;
    sigma2 = (float)(sg * sg);
  }
}

// 1 / c of coordinate j (j < D) of a row with (alpha, sigma^2)
__device__ __forceinline__ float mix_inv_c(const MixArgs& a, int j, float alpha, float sigma2) {
  const float g = a.G[j / a.C];
  const float v = a.var ? a.var[j] : 0.0f;
  const float c = (alpha * alpha) * v + sigma2 * (g * g);
  return 1.0f / c;
}

// v of the lane N places further round its 16-lane row (DPP row_ror: a register move, no LDS round trip)
template <int N>
__device__ __forceinline__ float row_ror(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xf, 0xf, false));
}
// All-reduce over a 16-lane row by rotations of 8, 4, 2, 1.  At every stage the two lanes of a pair add the same two
// values (in either order: fp32 addition commutes), so all 16 lanes end with the same bits.
__device__ __forceinline__ float group16_max(float v) {
  v = fmaxf(v, row_ror<8>(v));
  v = fmaxf(v, row_ror<4>(v));
  v = fmaxf(v, row_ror<2>(v));
  return fmaxf(v, row_ror<1>(v));
}
__device__ __forceinline__ float group16_sum(float v) {
  v = v + row_ror<8>(v);
  v = v + row_ror<4>(v);
  v = v + row_ror<2>(v);
  return v + row_ror<1>(v);
}

// NJ: float4 chunks of a row per lane; the padded row is DP = 64 NJ floats
// (No occupancy target: capped at 128 registers for four workgroups per CU the 192-coordinate instance spills 112 bytes
// per lane inside the tile loop and runs slower -- 0.196 against 0.112 ms at K = 4096 -- than two workgroups without spills.)
// VJP (ffd_mixture_score_vjp): the same pass with p'_i = (x - alpha mu_i) . q, q = v / c, formed next to the logit from
// the same difference, and two more sums carried through the online softmax: sum_i e_i p'_i and, on the matrix cores,
// sum_i e_i p'_i mu_i.  It leaves (max, sum, sum e p', sum e mu, sum e p' mu) per (slice, row).
template <int NJ, bool VJP>
__global__ __launch_bounds__(256) void k_mixture_part(MixArgs a) {
  constexpr int DP = 64 * NJ, DPS = DP + 16;  // (+16: the four component rows of an MFMA B read land on different banks)
  constexpr int NLD = KT * DP / 256;          // floats of a means tile per thread
  __shared__ __attribute__((aligned(16))) float mu[KT * DPS];
  constexpr int NS = VJP ? 2 : 1;  // images of the partial sums and of the weights: [0] the logit's, [1] p' and e p'
  __shared__ __attribute__((aligned(16))) float part[NS * RT * PART_STRIDE];
  __shared__ float P[NS * RT * KT];
  __shared__ __attribute__((aligned(16))) float scale[RT];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int grp = lane >> 4, t16 = lane & 15;
  const int row_l = 4 * w + grp;                 // the row of the tile this lane's vector work belongs to
  const int row = blockIdx.x * RT + row_l;
  const bool row_ok = row < a.B;
  const int D = a.D;
  const int k_begin = blockIdx.y * SL;
  const int k_end = min(a.K, k_begin + SL);

  float alpha = 1.0f, sigma2 = 1.0f;
  if (row_ok) mix_coeffs(a.sde, a.sa, a.sb, a.t[(size_t)row * a.t_stride], alpha, sigma2);

  // this lane's coordinates: chunk q holds j = (16 q + t16) 4 + e
  f32x2 xr[2 * NJ], ic[2 * NJ], qr[VJP ? 2 * NJ : 1];
#pragma unroll
  for (int q = 0; q < NJ; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = (16 * q + t16) * 4 + e;
      const bool ok = row_ok && j < D;
      xr[2 * q + (e >> 1)][e & 1] = ok ? a.x[(size_t)row * D + j] : 0.0f;
      ic[2 * q + (e >> 1)][e & 1] = ok ? mix_inv_c(a, j, alpha, sigma2) : 0.0f;
      if constexpr (VJP) qr[2 * q + (e >> 1)][e & 1] = ok ? a.v[(size_t)row * D + j] * ic[2 * q + (e >> 1)][e & 1] : 0.0f;
    }
  const f32x2 nal = {-alpha, -alpha};

  // a means tile, flat over (component, padded coordinate): element i 256 + tid
  float st[NLD];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = i * 256 + tid, c = idx / DP, j = idx - c * DP;
      st[i] = (k0 + c < k_end && j < D) ? a.means[(size_t)(k0 + c) * D + j] : 0.0f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = i * 256 + tid, c = idx / DP, j = idx - c * DP;
      mu[c * DPS + j] = st[i];
    }
  };

  f32x4 acc[NJ], accp[VJP ? NJ : 1];
#pragma unroll
  for (int n = 0; n < NJ; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (VJP)
#pragma unroll
    for (int n = 0; n < NJ; ++n) accp[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.0f, sp_run = 0.0f;
  const int wbase = w * 16 * NJ;  // the wave's quarter of the padded coordinates (MFMA phase)

  fetch(k_begin);
  stage();
  __syncthreads();
  for (int k0 = k_begin; k0 < k_end; k0 += KT) {
    const bool more = k0 + KT < k_end;
    if (more) fetch(k0 + KT);

    // ---- logits, difference form: sum_j t (t / c), t = x - alpha mu ----
    float ps[KT], pp[VJP ? KT : 1];
#pragma unroll
    for (int c = 0; c < KT; ++c) {
      f32x2 s2 = {0.f, 0.f}, s3 = {0.f, 0.f};
#pragma unroll
      for (int q = 0; q < NJ; ++q) {
        const float4 m4 = *reinterpret_cast<const float4*>(&mu[c * DPS + (16 * q + t16) * 4]);
        const f32x2 m01 = {m4.x, m4.y}, m23 = {m4.z, m4.w};
        const f32x2 t0 = nal * m01 + xr[2 * q], t1 = nal * m23 + xr[2 * q + 1];
        s2 = t0 * (t0 * ic[2 * q]) + s2;
        s2 = t1 * (t1 * ic[2 * q + 1]) + s2;
        if constexpr (VJP) {
          s3 = t0 * qr[2 * q] + s3;
          s3 = t1 * qr[2 * q + 1] + s3;
        }
      }
      ps[c] = s2.x + s2.y;
      if constexpr (VJP) pp[c] = s3.x + s3.y;
    }
#pragma unroll
    for (int c4 = 0; c4 < KT / 4; ++c4) {
      *reinterpret_cast<float4*>(&part[row_l * PART_STRIDE + t16 * KT + 4 * c4]) =
          make_float4(ps[4 * c4], ps[4 * c4 + 1], ps[4 * c4 + 2], ps[4 * c4 + 3]);
      if constexpr (VJP)
        *reinterpret_cast<float4*>(&part[(RT + row_l) * PART_STRIDE + t16 * KT + 4 * c4]) =
            make_float4(pp[4 * c4], pp[4 * c4 + 1], pp[4 * c4 + 2], pp[4 * c4 + 3]);
    }
    __syncthreads();

    // ---- lane (row, component t16): the row's 16 partial sums in lane order, then the online softmax ----
    float sq = 0.0f;
#pragma unroll
    for (int u = 0; u < 16; ++u) sq += part[row_l * PART_STRIDE + u * KT + t16];
    const int comp = k0 + t16;
    const float logit = comp < k_end ? a.logw[comp] - 0.5f * sq : -INFINITY;
    const float m_new = fmaxf(m_run, group16_max(logit));
    // (everything so far at -inf: no weight yet, the accumulators hold zeros and stay as they are)
    const float p = m_new == -INFINITY ? 0.0f : expf(logit - m_new);
    const float sc = (m_new == -INFINITY || m_run == -INFINITY) ? 1.0f : expf(m_run - m_new);
    l_run = l_run * sc + group16_sum(p);
    m_run = m_new;
    P[row_l * KT + t16] = p;
    if constexpr (VJP) {
      float pv = 0.0f;
#pragma unroll
      for (int u = 0; u < 16; ++u) pv += part[(RT + row_l) * PART_STRIDE + u * KT + t16];
      const float ep = p * pv;  // (a component without weight, or past the slice's end: p = 0, pv finite)
      sp_run = sp_run * sc + group16_sum(ep);
      P[(RT + row_l) * KT + t16] = ep;
    }
    if (t16 == 0) scale[row_l] = sc;
    __syncthreads();

    // ---- sum_i p_i mu_i on the matrix cores: A = P (row l & 15, component 4 kk + (l >> 4)), B = mu ----
    {
      const float4 s4 = *reinterpret_cast<const float4*>(&scale[4 * grp]);  // the accumulator rows 4 (l >> 4) + r
#pragma unroll
      for (int n = 0; n < NJ; ++n) {
        acc[n][0] *= s4.x;
        acc[n][1] *= s4.y;
        acc[n][2] *= s4.z;
        acc[n][3] *= s4.w;
      }
      if constexpr (VJP)
#pragma unroll
        for (int n = 0; n < NJ; ++n) {
          accp[n][0] *= s4.x;
          accp[n][1] *= s4.y;
          accp[n][2] *= s4.z;
          accp[n][3] *= s4.w;
        }
#pragma unroll
      for (int kk = 0; kk < KT / 4; ++kk) {
        const float pa = P[t16 * KT + 4 * kk + grp];
        if constexpr (VJP) {
          const float pb = P[(RT + t16) * KT + 4 * kk + grp];
#pragma unroll
          for (int n = 0; n < NJ; ++n) {
            const float m = mu[(4 * kk + grp) * DPS + wbase + 16 * n + t16];
            acc[n] = mfma16(pa, m, acc[n]);
            accp[n] = mfma16(pb, m, accp[n]);
          }
        } else {
#pragma unroll
          for (int n = 0; n < NJ; ++n) acc[n] = mfma16(pa, mu[(4 * kk + grp) * DPS + wbase + 16 * n + t16], acc[n]);
        }
      }
    }
    __syncthreads();
    if (more) {
      stage();
      __syncthreads();
    }
  }

  // ---- the slice's partial: (max, sum, weighted sum) per row; VJP: (max, sum, sum e p', sum e mu, sum e p' mu) ----
  constexpr int HD = VJP ? 3 : 2;
  const size_t DS = VJP ? 2 * (size_t)D + 3 : (size_t)D + 2;
  float* const wslice = a.work + (size_t)blockIdx.y * a.B * DS;
  if (row_ok && t16 == 0) {
    wslice[(size_t)row * DS] = m_run;
    wslice[(size_t)row * DS + 1] = l_run;
    if constexpr (VJP) wslice[(size_t)row * DS + 2] = sp_run;
  }
#pragma unroll
  for (int n = 0; n < NJ; ++n) {
    const int j = wbase + 16 * n + t16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = blockIdx.x * RT + 4 * grp + r;
      if (orow < a.B && j < D) {
        wslice[(size_t)orow * DS + HD + j] = acc[n][r];
        if constexpr (VJP) wslice[(size_t)orow * DS + HD + D + j] = accp[n][r];
      }
    }
  }
}

// One workgroup per row: the slices in ascending order, then d = alpha mean - x and score = d / c.
__global__ __launch_bounds__(256) void k_mixture_merge(MixArgs a, int nslice) {
  const int row = blockIdx.x, D = a.D;
  const size_t DS = (size_t)D + 2, SS = (size_t)a.B * DS;
  const float* const wr = a.work + (size_t)row * DS;
  float alpha, sigma2;
  mix_coeffs(a.sde, a.sa, a.sb, a.t[(size_t)row * a.t_stride], alpha, sigma2);
  float M = -INFINITY;
  for (int s = 0; s < nslice; ++s) M = fmaxf(M, wr[s * SS]);
  float lsum = 0.0f;
  for (int s = 0; s < nslice; ++s) {
    const float ms = wr[s * SS];
    lsum += wr[s * SS + 1] * (ms == -INFINITY ? 0.0f : expf(ms - M));
  }
  const float inv_l = lsum > 0.0f ? 1.0f / lsum : 0.0f;  // (no component with weight: the mean term drops out)
  for (int j = threadIdx.x; j < D; j += blockDim.x) {
    float mean = 0.0f;
    for (int s = 0; s < nslice; ++s) {
      const float ms = wr[s * SS];
      mean += wr[s * SS + 2 + j] * (ms == -INFINITY ? 0.0f : expf(ms - M));
    }
    mean *= inv_l;
    const float d = alpha * mean - a.x[(size_t)row * D + j];
    a.out[(size_t)row * D + j] = d * mix_inv_c(a, j, alpha, sigma2);
  }
}

// The VJP's merge.  J = d score / d x is symmetric: J_jk = alpha^2 Cov_r(mu_j, mu_k) / (c_j c_k) - delta_jk / c_j.  With
// p'_i = (x - alpha mu_i) . q = -alpha (mu_i - x / alpha) . q (the covariance does not see the shift):
//   (J^T v)_j = -(alpha / c_j) (sum_i r_i p'_i mu_ij - mean_j sum_i r_i p'_i) - q_j,   q = v / c.
__global__ __launch_bounds__(256) void k_mixture_vjp_merge(MixArgs a, int nslice) {
  const int row = blockIdx.x, D = a.D;
  const size_t DS = 2 * (size_t)D + 3, SS = (size_t)a.B * DS;
  const float* const wr = a.work + (size_t)row * DS;
  float alpha, sigma2;
  mix_coeffs(a.sde, a.sa, a.sb, a.t[(size_t)row * a.t_stride], alpha, sigma2);
  float M = -INFINITY;
  for (int s = 0; s < nslice; ++s) M = fmaxf(M, wr[s * SS]);
  float lsum = 0.0f, psum = 0.0f;
  for (int s = 0; s < nslice; ++s) {
    const float ms = wr[s * SS], f = ms == -INFINITY ? 0.0f : expf(ms - M);
    lsum += wr[s * SS + 1] * f;
    psum += wr[s * SS + 2] * f;
  }
  const float inv_l = lsum > 0.0f ? 1.0f / lsum : 0.0f;  // (no component with weight: the covariance term drops out)
  const float pbar = psum * inv_l;
  for (int j = threadIdx.x; j < D; j += blockDim.x) {
    float mean = 0.0f, pm = 0.0f;
    for (int s = 0; s < nslice; ++s) {
      const float ms = wr[s * SS], f = ms == -INFINITY ? 0.0f : expf(ms - M);
      mean += wr[s * SS + 3 + j] * f;
      pm += wr[s * SS + 3 + D + j] * f;
    }
    const float icj = mix_inv_c(a, j, alpha, sigma2);
    // (fp32 on purpose: with one component the two products round alike and the covariance is an exact zero)
    const float cov = __fsub_rn(__fmul_rn(pm, inv_l), __fmul_rn(__fmul_rn(mean, inv_l), pbar));
    a.out[(size_t)row * D + j] = -(alpha * icj) * cov - a.v[(size_t)row * D + j] * icj;
  }
}

__global__ void k_mixture_times(const float* ts, float t_imm, int n, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = ts ? ts[i] : t_imm;
}

int mix_nslice(int K) { return cdiv(K, SL); }

}  // namespace

bool mixture_shape_supported(int B, int K, int L, int C) {
  if (B < 1 || K < 1 || L < 1 || C < 1) return false;
  if ((int64_t)L * C > MIX_MAX_DIM) return false;
  if (mix_nslice(K) > 65535) return false;                                   // gridDim.y
  if ((int64_t)B * ((int64_t)L * C + 2) * mix_nslice(K) > (int64_t)1 << 40) return false;
  return (int64_t)B * L * C < ((int64_t)1 << 31) && (int64_t)K * L * C < ((int64_t)1 << 40);
}

size_t mixture_work_floats(int B, int K, int L, int C) {
  if (!mixture_shape_supported(B, K, L, C)) return 0;
  return (size_t)mix_nslice(K) * (size_t)B * ((size_t)L * C + 2);
}

size_t mixture_vjp_work_floats(int B, int K, int L, int C) {
  if (!mixture_shape_supported(B, K, L, C)) return 0;
  return (size_t)mix_nslice(K) * (size_t)B * (2 * (size_t)L * C + 3);
}

hipError_t launch_mixture_score(int sde, double sa, double sb, const float* x, const float* t, int t_stride,
                                const float* means, const float* logw, const float* var, const float* G, float* out, int B,
                                int K, int L, int C, float* work, hipStream_t s) {
  if (!mixture_shape_supported(B, K, L, C)) return hipErrorInvalidValue;
  const int D = L * C, nslice = mix_nslice(K);
  MixArgs a{x, t, means, logw, var, G, work, out, sa, sb, sde, t_stride, B, K, L, C, D, nullptr};
  const dim3 grid(cdiv(B, RT), nslice);
  if (D <= 64) hipLaunchKernelGGL((k_mixture_part<1, false>), grid, dim3(256), 0, s, a);
  else if (D <= 192) hipLaunchKernelGGL((k_mixture_part<3, false>), grid, dim3(256), 0, s, a);
  else if (D <= 256) hipLaunchKernelGGL((k_mixture_part<4, false>), grid, dim3(256), 0, s, a);
  else if (D <= 512) hipLaunchKernelGGL((k_mixture_part<8, false>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_mixture_part<16, false>), grid, dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mixture_merge, dim3(B), dim3(256), 0, s, a, nslice);
  return hipGetLastError();
}

hipError_t launch_mixture_score_vjp(int sde, double sa, double sb, const float* x, const float* t, int t_stride,
                                    const float* means, const float* logw, const float* var, const float* G, const float* v,
                                    float* out, int B, int K, int L, int C, float* work, hipStream_t s) {
  if (!mixture_shape_supported(B, K, L, C)) return hipErrorInvalidValue;
  const int D = L * C, nslice = mix_nslice(K);
  MixArgs a{x, t, means, logw, var, G, work, out, sa, sb, sde, t_stride, B, K, L, C, D, v};
  const dim3 grid(cdiv(B, RT), nslice);
  if (D <= 64) hipLaunchKernelGGL((k_mixture_part<1, true>), grid, dim3(256), 0, s, a);
  else if (D <= 192) hipLaunchKernelGGL((k_mixture_part<3, true>), grid, dim3(256), 0, s, a);
  else if (D <= 256) hipLaunchKernelGGL((k_mixture_part<4, true>), grid, dim3(256), 0, s, a);
  else if (D <= 512) hipLaunchKernelGGL((k_mixture_part<8, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_mixture_part<16, true>), grid, dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mixture_vjp_merge, dim3(B), dim3(256), 0, s, a, nslice);
  return hipGetLastError();
}

hipError_t launch_mixture_times(const float* ts, float t_imm, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_mixture_times, dim3(cdiv(n, 256)), dim3(256), 0, s, ts, t_imm, n, out);
  return hipGetLastError();
}

int mixture_check(const float* means, const float* logw, const float* var, int K, int L, int C, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "";
  if (!means || !logw || K < 1 || L < 1 || C < 1) return *why = "a null pointer or K, L, C < 1", FFD_ERR_INVALID;
  if ((int64_t)L * C > MIX_MAX_DIM) return *why = "L * C above the mixture kernel's limit", FFD_ERR_UNSUPPORTED;
  const size_t D = (size_t)L * C;
  for (size_t i = 0; i < (size_t)K * D; ++i)
    if (!std::isfinite(means[i])) return *why = "a non-finite mean", FFD_ERR_INVALID;
  if (var)
    for (size_t i = 0; i < D; ++i)
      if (!(var[i] >= 0.0f) || !std::isfinite(var[i])) return *why = "a negative or non-finite variance", FFD_ERR_INVALID;
  bool any = false;
  for (int i = 0; i < K; ++i) {
    if (std::isnan(logw[i]) || logw[i] == INFINITY) return *why = "a NaN or +inf log-weight", FFD_ERR_INVALID;
    any = any || logw[i] != -INFINITY;
  }
  if (!any) return *why = "every log-weight is -inf", FFD_ERR_INVALID;
  return FFD_OK;
}

}  // namespace ffd

// ---- C ABI (include/ffd.h) ----
using namespace ffd;

extern "C" {

size_t ffd_mixture_work_floats(int B, int K, int L, int C) { return mixture_work_floats(B, K, L, C); }

int ffd_mixture_tiling(int* row_tile, int* comp_tile, int* slice, int* max_dim) {
  if (row_tile) *row_tile = MIX_ROW_TILE;
  if (comp_tile) *comp_tile = MIX_COMP_TILE;
  if (slice) *slice = MIX_SLICE;
  if (max_dim) *max_dim = MIX_MAX_DIM;
  return FFD_OK;
}

size_t ffd_mixture_vjp_work_floats(int B, int K, int L, int C) { return mixture_vjp_work_floats(B, K, L, C); }

int ffd_mixture_score_vjp(const ffd_sde_desc* sde, const float* x, const float* t, int t_stride, const float* means,
                          const float* log_weights, const float* variance, const float* G, const float* v, float* out,
                          int B, int K, int L, int C, float* work, size_t work_floats, void* stream) {
  if (!sde || !x || !t || !means || !log_weights || !G || !v || !out || !work) return FFD_ERR_INVALID;
  if (B < 1 || K < 1 || L < 1 || C < 1 || (t_stride != 0 && t_stride != 1)) return FFD_ERR_INVALID;
  if (sde->sde != FFD_SDE_VP && sde->sde != FFD_SDE_VE) return FFD_ERR_UNSUPPORTED;
  if (!mixture_shape_supported(B, K, L, C)) return FFD_ERR_UNSUPPORTED;
  if (work_floats < mixture_vjp_work_floats(B, K, L, C)) return FFD_ERR_INVALID;
  hipError_t e = launch_mixture_score_vjp(sde->sde, sde->a, sde->b, x, t, t_stride, means, log_weights, variance, G, v, out,
                                          B, K, L, C, work, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_host_mixture_check(const float* means, const float* log_weights, const float* variance, int K, int L, int C) {
  return mixture_check(means, log_weights, variance, K, L, C, nullptr);
}

int ffd_mixture_score(const ffd_sde_desc* sde, const float* x, const float* t, int t_stride, const float* means,
                      const float* log_weights, const float* variance, const float* G, float* score_out, int B, int K,
                      int L, int C, float* work, size_t work_floats, void* stream) {
  if (!sde || !x || !t || !means || !log_weights || !G || !score_out || !work) return FFD_ERR_INVALID;
  if (B < 1 || K < 1 || L < 1 || C < 1 || (t_stride != 0 && t_stride != 1)) return FFD_ERR_INVALID;
  if (sde->sde != FFD_SDE_VP && sde->sde != FFD_SDE_VE) return FFD_ERR_UNSUPPORTED;
  if (!mixture_shape_supported(B, K, L, C)) return FFD_ERR_UNSUPPORTED;
  if (work_floats < mixture_work_floats(B, K, L, C)) return FFD_ERR_INVALID;
  hipError_t e = launch_mixture_score(sde->sde, sde->a, sde->b, x, t, t_stride, means, log_weights, variance, G, score_out,
                                      B, K, L, C, work, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"
