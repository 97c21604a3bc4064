// Localization metrics, frequency smoothing and per-dataset spectral profiles on the device
// (fdiff.utils.fourier.localization_metrics / smooth_frequency, fourier.py:134-216, and the statistics of
// fdiff.visualization.spectral_interpretation.process_dataset, spectral_interpretation.py:55-94).
//
//   k_norm_rows      per sample: the channel-summed energy (x^2) or density rows, optionally mirrored to the full
//                    length-L frequency axis (fourier.py:154-159), divided by their fp64 total (fourier.py:147-163)
//   k_deloc          min_s sum_t p[t] cyc(t, s)^2 for the 2 B normalized rows on the fp32 16x16x4 MFMA: the cyc^2
//                    operand is made from the lane's indices, the minimum over centres stays in registers / LDS
//   k_smooth_kernel  the column-normalized Gaussian kernel of smooth_frequency (fourier.py:201-210), L x L
//   k_smooth_mm      Y[b, s, c] = sum_t Xf[b, t, c] W[t, s] on the same MFMA, W shared by the whole batch
//   k_prof_*         batch mean and unbiased batch std of the normalized rows: two passes over fixed 1024-sample slabs
//
// Every reduction is a fixed-order fp64 tree (or, inside the MFMA, the fixed chain over t) with no atomics: a sample's
// result depends on its own rows only.  The ffd_localization / ffd_smooth_frequency / ffd_spectral_profile entry points
// follow the kernels.
#include <math.h>

#include <algorithm>
#include <cmath>

#include "ffd_internal.h"

namespace ffd {

// ---- normalized rows -------------------------------------------------------------------------------------------
// One workgroup per sample.  in: (B, n, C).  e[k] = sum_c v (sq: v = in^2, else in), summed in fp64 in channel order.
// mirror_L == 0: p[k] = e[k] / sum_k e[k], k < n.  mirror_L == L: in holds the n = L/2 + 1 density bins; the row is
// continued by the flipped bins 1 .. (L odd ? n - 1 : n - 2) (fourier.py:154-159), so p[j] = e[j < n ? j : L - j] / total
// with the total over all L entries.  An all-zero sample gives 0 / 0 = NaN like the reference.  The rows are evaluated
// twice (total, then quotient) instead of being kept: a sample's slab stays in L2 between the two.
__device__ __forceinline__ double row_energy(const float* __restrict__ src, int k, int C, bool sq) {
  const float* p = src + (size_t)k * C;
  double e = 0.0;
  for (int c = 0; c < C; ++c) {
    const double v = (double)p[c];
    e += sq ? v * v : v;
  }
  return e;
}

__global__ __launch_bounds__(256) void k_norm_rows(const float* __restrict__ in, int n, int C, int sq, int mirror_L,
                                                   float* __restrict__ p_out, double* __restrict__ tot_out) {
  __shared__ double red[256];
  const size_t b = blockIdx.x;
  const float* src = in + b * (size_t)n * C;
  const int L = mirror_L;
  double acc = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) {
    const double e = row_energy(src, k, C, sq != 0);
    const bool twice = L > 0 && k >= 1 && L - k >= n;  // the bin has a mirrored twin at L - k
    acc += twice ? 2.0 * e : e;
  }
  const double total = block_sum(acc, red);
  const int nout = L > 0 ? L : n;
  float* dst = p_out + b * (size_t)nout;
  for (int j = threadIdx.x; j < nout; j += 256) {
    const int k = j < n ? j : L - j;
    dst[j] = (float)(row_energy(src, k, C, sq != 0) / total);
  }
  if (tot_out && threadIdx.x == 0) tot_out[b] = total;
}

static hipError_t launch_norm_rows(const float* in, int B, int n, int C, int sq, int mirror_L, float* p_out,
                                   double* tot_out, hipStream_t s) {
  hipLaunchKernelGGL(k_norm_rows, dim3(B), dim3(256), 0, s, in, n, C, sq, mirror_L, p_out, tot_out);
  return hipGetLastError();
}

// ---- delocalization: min over centres of the cyclic second moment ----------------------------------------------
// NaN-keeping minimum: a NaN on either side stays (the reference's torch.min propagates it)
__device__ __forceinline__ float min_nan(float v, float m) { return (v < m || v != v) ? v : m; }

// A workgroup (4 waves) owns DL_ROWS = 32 rows of P (R, L) as two 16-row MFMA tiles; wave w takes the centre tiles
// w, w + 4, ...  A = P (i = row, k = t), B[k = t][j = s] = cyc(t, s)^2 = min(|t - s|, L - |t - s|)^2, an integer below
// 2^24 for L <= 8192 and so exact in fp32; one B value feeds both row tiles.  LDSA: the row block sits in LDS (row
// stride ld, zero beyond L and beyond R) and every centre tile re-reads it from there; otherwise (rows too long for
// LDS) the A values come straight from HBM / L2.  t past L multiplies a zero; a centre past L is never taken into the
// minimum; rows past R are computed on zeros (LDS) or on a clamped row and never stored.
// The moment is a sum of L non-negative terms; in one fp32 accumulator chain its rounding error grows like sqrt(L) and
// reaches 2e-6 .. 5e-6 of the value at L = 6823 .. 8192 (measured), past the 2e-6 the time-domain value is held to.
// So the chain restarts every DL_SEG positions and the segment sums are added up: ~DL_SEG / sqrt(3 L) + sqrt(L / (3
// DL_SEG)) roundings' worth, below 3e-7 at every supported length.  L <= DL_SEG: one segment, the same bits as one chain.
constexpr int DL_ROWS = 32, DL_SEG = 256;

template <bool LDSA>
__global__ __launch_bounds__(256) void k_deloc(const float* __restrict__ P, float* __restrict__ out, int R, int L, int ld) {
  extern __shared__ __align__(16) float dl_sm[];
  float* red = dl_sm;             // [4][DL_ROWS]
  float* tile = dl_sm + 4 * DL_ROWS;  // [DL_ROWS][ld] (LDSA)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int r0 = blockIdx.x * DL_ROWS;
  if (LDSA) {  // wave w stages the rows w, w + 4, ...: 64 consecutive floats per load, no index arithmetic beyond t
    for (int rr = wave; rr < DL_ROWS; rr += 4) {
      const bool row_live = r0 + rr < R;
      const float* src = P + (size_t)min(r0 + rr, R - 1) * L;
      float* dst = tile + rr * ld;
      for (int t = lane; t < ld; t += 64) dst[t] = (row_live && t < L) ? src[t] : 0.f;
    }
    __syncthreads();
  }
  const float* g0 = P + (size_t)min(r0 + c, R - 1) * L;
  const float* g1 = P + (size_t)min(r0 + 16 + c, R - 1) * L;
  const float* l0 = tile + c * ld;
  const float* l1 = tile + (16 + c) * ld;
  float m0[4], m1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) m0[r] = m1[r] = INFINITY;
  const int nst = cdiv(L, 16);
  for (int st = wave; st < nst; st += 4) {
    const int s = st * 16 + c;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int tb = 0; tb < L; tb += DL_SEG) {  // one accumulator chain per DL_SEG positions, the segments added in order
      f32x4 seg0 = {0.f, 0.f, 0.f, 0.f}, seg1 = {0.f, 0.f, 0.f, 0.f};
      const int te = min(tb + DL_SEG, L);
      for (int t0 = tb; t0 < te; t0 += 4) {
        const int t = t0 + q;
        const int d = abs(t - s);
        const int cy = min(d, L - d);
        const float bv = (float)(cy * cy);
        float a0, a1;
        if (LDSA) {
          a0 = l0[t];
          a1 = l1[t];
        } else {
          a0 = t < L ? g0[t] : 0.f;
          a1 = t < L ? g1[t] : 0.f;
        }
        seg0 = mfma16(a0, bv, seg0);
        seg1 = mfma16(a1, bv, seg1);
      }
      acc0 += seg0;
      acc1 += seg1;
    }
    if (s < L) {  // D[i = 4 q + r][j = c]: row 16 a + 4 q + r, centre s
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        m0[r] = min_nan(acc0[r], m0[r]);
        m1[r] = min_nan(acc1[r], m1[r]);
      }
    }
  }
  // over the 16 centre lanes of a row, then over the waves in wave order
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      m0[r] = min_nan(__shfl_xor(m0[r], off), m0[r]);
      m1[r] = min_nan(__shfl_xor(m1[r], off), m1[r]);
    }
    if (c == 0) {
      red[wave * DL_ROWS + 4 * q + r] = m0[r];
      red[wave * DL_ROWS + 16 + 4 * q + r] = m1[r];
    }
  }
  __syncthreads();
  if (threadIdx.x < DL_ROWS && r0 + (int)threadIdx.x < R) {
    float m = red[threadIdx.x];
    for (int w = 1; w < 4; ++w) m = min_nan(red[w * DL_ROWS + threadIdx.x], m);
    out[r0 + threadIdx.x] = m;
  }
}

constexpr size_t DL_LDS_CAP = 144 * 1024;
static int deloc_ld(int L) { return lds_stride(4 * cdiv(L, 4)); }
static size_t deloc_lds_bytes(int L) { return (size_t)(4 * DL_ROWS + (size_t)DL_ROWS * deloc_ld(L)) * sizeof(float); }

// out[r] = min_s sum_t P[r, t] cyc(t, s)^2 for the R rows of P (R, L)
static hipError_t launch_deloc(const float* P, float* out, int R, int L, hipStream_t s) {
  const size_t lds = deloc_lds_bytes(L);
  const dim3 grid(cdiv(R, DL_ROWS)), block(256);
  if (lds <= DL_LDS_CAP) {
    static bool attr_set = false;  // once: the cap covers every length this branch takes
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_deloc<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)DL_LDS_CAP);
      if (e != hipSuccess) return e;
      attr_set = true;
    }
    hipLaunchKernelGGL(k_deloc<true>, grid, block, lds, s, P, out, R, L, deloc_ld(L));
  } else {
    hipLaunchKernelGGL(k_deloc<false>, grid, block, 4 * DL_ROWS * sizeof(float), s, P, out, R, L, 0);
  }
  return hipGetLastError();
}

// ---- smooth_frequency -------------------------------------------------------------------------------------------
// k (fourier.py:201-206) for odd L: [0 .. (L-1)/2, 1 .. (L-1)/2], the harmonic of packed position i
__device__ __forceinline__ float packed_harmonic(int i, int nr) { return (float)(i < nr ? i : i - nr + 1); }

// Column s of W (L x L row-major): W[t, s] = g(t, s) / sum_t g(t, s), g = exp(-((k_t - k_s) / sigma)^2 / 2) in fp32 like
// the reference (fourier.py:209-210); the column sum in fp64 in a fixed order.
__global__ __launch_bounds__(256) void k_smooth_kernel(float* __restrict__ W, int L, float sigma) {
  __shared__ double red[256];
  const int s = blockIdx.x, nr = (L + 1) / 2;
  const float ks = packed_harmonic(s, nr);
  double acc = 0.0;
  for (int t = threadIdx.x; t < L; t += 256) {
    const float z = __fdiv_rn(__fsub_rn(packed_harmonic(t, nr), ks), sigma);
    acc += (double)expf(-__fmul_rn(z, z) / 2.f);
  }
  const double total = block_sum(acc, red);
  for (int t = threadIdx.x; t < L; t += 256) {
    const float z = __fdiv_rn(__fsub_rn(packed_harmonic(t, nr), ks), sigma);
    W[(size_t)t * L + s] = (float)((double)expf(-__fmul_rn(z, z) / 2.f) / total);
  }
}

// Y[b, s, c] = sum_t Xf[b, t, c] W[t, s] (the einsum of fourier.py:214).  A workgroup owns 16 series n = b C + c and
// every output position; wave w takes the position tiles w, w + 4, ...  A[i = s][k = t] = W[t, s] (16 consecutive
// floats per k: coalesced, L2-resident), B[k = t][j = n] = Xf[b, t, c].  t past L: both operands zero; positions
// past L and series past N are clamped for the loads and never stored.
__global__ __launch_bounds__(256) void k_smooth_mm(const float* __restrict__ Xf, const float* __restrict__ W,
                                                   float* __restrict__ Y, int N, int L, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int n = min((int)blockIdx.x * 16 + c, N - 1);
  const bool live = (int)blockIdx.x * 16 + c < N;
  const int b = n / C, ch = n - b * C;
  const float* xcol = Xf + (size_t)b * L * C + ch;
  float* ycol = Y + (size_t)b * L * C + ch;
  const int nst = cdiv(L, 16);
  for (int st = wave; st < nst; st += 4) {
    const float* wcol = W + min(st * 16 + c, L - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < L; t0 += 4) {
      const int t = t0 + q;
      const int tc = min(t, L - 1);
      const float a = t < L ? wcol[(size_t)tc * L] : 0.f;
      const float bv = t < L ? xcol[(size_t)tc * C] : 0.f;
      acc = mfma16(a, bv, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // D[i = 4 q + r][j = c]: position 16 st + 4 q + r of series n
      const int so = st * 16 + 4 * q + r;
      if (live && so < L) ycol[(size_t)so * C] = acc[r];
    }
  }
}

// ---- batch statistics of the normalized rows --------------------------------------------------------------------
// spectral_interpretation.py:58-68,85-94: the mean over the batch of e / (EPS + total) and the unbiased std over the
// batch of e / total (EPS = 1e-15 enters the mean's denominator only).  p (B, n) holds e / total, tot (B) the totals.
// Slabs of PF_SLAB samples: a workgroup sums 64 positions of one slab in fp64 (4 sample groups, combined in order),
// then one thread per position adds the slabs in order.  The slab size is fixed, so the grid never changes a result.
constexpr int PF_SLAB = 1024;
constexpr double PF_EPS = 1e-15;

// part[slab][0][k] = sum_b p e-term (with EPS), part[slab][1][k] = sum_b p (mean_p == nullptr);
// with mean_p: part[slab][0][k] = sum_b (p - mean_p[k])^2
__global__ __launch_bounds__(256) void k_prof_partial(const float* __restrict__ p, const double* __restrict__ tot,
                                                      const double* __restrict__ mean_p, int B, int n,
                                                      double* __restrict__ part) {
  __shared__ double red[2][4][64];
  const int cl = threadIdx.x & 63, k = blockIdx.x * 64 + cl, g = threadIdx.x >> 6;
  const int b0 = blockIdx.y * PF_SLAB, b1 = min(b0 + PF_SLAB, B);
  double s0 = 0.0, s1 = 0.0;
  if (k < n) {
    if (mean_p) {
      const double mu = mean_p[k];
      for (int b = b0 + g; b < b1; b += 4) {
        const double d = (double)p[(size_t)b * n + k] - mu;
        s0 += d * d;
      }
    } else {
      for (int b = b0 + g; b < b1; b += 4) {
        const double v = (double)p[(size_t)b * n + k], t = tot[b];
        s0 += t > 0.0 ? v * (t / (PF_EPS + t)) : 0.0;  // e / (EPS + total); an all-zero sample adds 0 / EPS = 0
        s1 += v;
      }
    }
  }
  red[0][g][cl] = s0;
  red[1][g][cl] = s1;
  __syncthreads();
  if (g == 0 && k < n) {
    double* dst = part + (size_t)blockIdx.y * 2 * n;
    dst[k] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
    dst[n + k] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
  }
}

// pass 1 (std_out == nullptr): mean_out[k] = sum / B (fp32), mean_p[k] = plain mean (fp64, for pass 2);
// pass 2: std_out[k] = sqrt(sum / (B - 1)) * scale  (B == 1: 0 / 0 = NaN like torch.std)
__global__ __launch_bounds__(256) void k_prof_final(const double* __restrict__ part, int nslab, int B, int n,
                                                    float* __restrict__ mean_out, double* __restrict__ mean_p,
                                                    float* __restrict__ std_out, double scale) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  double s0 = 0.0, s1 = 0.0;
  for (int i = 0; i < nslab; ++i) {
    s0 += part[(size_t)i * 2 * n + k];
    s1 += part[(size_t)i * 2 * n + n + k];
  }
  if (std_out) {
    std_out[k] = (float)(sqrt(s0 / (double)(B - 1)) * scale);
  } else {
    mean_out[k] = (float)(s0 / (double)B);
    mean_p[k] = s1 / (double)B;
  }
}

// part: nslab * 2 * n doubles, mean_p: n doubles
static hipError_t launch_profile(const float* p, const double* tot, int B, int n, float* mean_out, float* std_out,
                                 double scale, double* part, double* mean_p, hipStream_t s) {
  const int nslab = cdiv(B, PF_SLAB);
  const dim3 gp(cdiv(n, 64), nslab), gf(cdiv(n, 256)), block(256);
  hipLaunchKernelGGL(k_prof_partial, gp, block, 0, s, p, tot, (const double*)nullptr, B, n, part);
  hipLaunchKernelGGL(k_prof_final, gf, block, 0, s, part, nslab, B, n, mean_out, mean_p, (float*)nullptr, 1.0);
  hipLaunchKernelGGL(k_prof_partial, gp, block, 0, s, p, tot, (const double*)mean_p, B, n, part);
  hipLaunchKernelGGL(k_prof_final, gf, block, 0, s, part, nslab, B, n, (float*)nullptr, (double*)nullptr, std_out, scale);
  return hipGetLastError();
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): localization metrics, frequency smoothing, spectral profiles ----
using namespace ffd;

extern "C" {

// Limits: the FFT's own lengths (fft_len_supported: powers of two up to 8192, any other L up to 6826; cyc^2 < 2^24 is
// exact in fp32 for all of them), smoothing L <= 2047 (the L x L kernel), B <= 2^24 samples, C <= 2^16 channels per
// call (FFD_ERR_UNSUPPORTED past them, before any device call; the matching *_work_bytes is then 0).
static const int SP_MAX_L = FFT_MAX_LEN, SP_MAX_SMOOTH_L = 2047, SP_MAX_B = 1 << 24, SP_MAX_C = 1 << 16;

static int sp_check(int B, int L, int C, int max_len = SP_MAX_L) {
  if (B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  if (!fft_len_supported(L, max_len) || B > SP_MAX_B || C > SP_MAX_C) return FFD_ERR_UNSUPPORTED;
  return FFD_OK;
}

// floats of the spectrum (B, L, C) and of the density (B, L/2 + 1, C)
static size_t sp_spec_floats(int B, int L, int C) { return (size_t)B * L * C + (size_t)B * (L / 2 + 1) * C; }

// x -> packed spectrum -> density (B, L/2 + 1, C) in `dens`
static int sp_density(const float* x, float* xf, float* dens, int B, int L, int C, void* stream) {
  if (int rc = ffd_dft(x, xf, B, L, C, stream)) return rc;
  return ffd_spectral_density(xf, dens, B, L, C, stream);
}

size_t ffd_localization_work_bytes(int B, int L, int C) {
  if (sp_check(B, L, C) != FFD_OK) return 0;
  return (sp_spec_floats(B, L, C) + 2 * (size_t)B * L) * sizeof(float);
}

// The stages of ffd_localization, shared with ffd_localization_bench.  ev (optional, 4 events) is recorded in front of
// the time-domain rows, of the transform, of the products and behind them.
static int localization_stages(const float* x, float* deloc_time_out, float* deloc_freq_out, void* work, int B, int L,
                               int C, void* stream, hipEvent_t* ev) {
  hipStream_t s = (hipStream_t)stream;
  float* xf = (float*)work;
  float* dens = xf + (size_t)B * L * C;
  float* P = dens + (size_t)B * (L / 2 + 1) * C;  // rows [0, B): time, [B, 2 B): frequency
  if (ev && hipEventRecord(ev[0], s) != hipSuccess) return FFD_ERR_HIP;
  if (launch_norm_rows(x, B, L, C, 1, 0, P, nullptr, s) != hipSuccess) return FFD_ERR_HIP;
  if (ev && hipEventRecord(ev[1], s) != hipSuccess) return FFD_ERR_HIP;
  if (int rc = sp_density(x, xf, dens, B, L, C, stream)) return rc;
  if (launch_norm_rows(dens, B, L / 2 + 1, C, 0, L, P + (size_t)B * L, nullptr, s) != hipSuccess) return FFD_ERR_HIP;
  if (ev && hipEventRecord(ev[2], s) != hipSuccess) return FFD_ERR_HIP;
  // one product launch per output array: the two need not be adjacent
  if (launch_deloc(P, deloc_time_out, B, L, s) != hipSuccess) return FFD_ERR_HIP;
  if (launch_deloc(P + (size_t)B * L, deloc_freq_out, B, L, s) != hipSuccess) return FFD_ERR_HIP;
  if (ev && hipEventRecord(ev[3], s) != hipSuccess) return FFD_ERR_HIP;
  return FFD_OK;
}

int ffd_localization(const float* x, float* deloc_time_out, float* deloc_freq_out, void* work, size_t work_bytes, int B,
                     int L, int C, void* stream) {
  if (!x || !deloc_time_out || !deloc_freq_out || !work) return FFD_ERR_INVALID;
  if (int rc = sp_check(B, L, C)) return rc;
  if (work_bytes < ffd_localization_work_bytes(B, L, C)) return FFD_ERR_INVALID;
  return localization_stages(x, deloc_time_out, deloc_freq_out, work, B, L, C, stream, nullptr);
}

// The longest row whose 32-row block the product kernel keeps in LDS; longer rows are read from L2 per centre tile.
int ffd_localization_lds_max_len(void) {
  int L = 1;
  while (L < SP_MAX_L && deloc_lds_bytes(L + 1) <= DL_LDS_CAP) ++L;
  return L;
}

size_t ffd_smooth_frequency_work_bytes(int B, int L, int C) {
  if (sp_check(B, L, C, SP_MAX_SMOOTH_L) != FFD_OK || L % 2 == 0 || (long long)B * C > (1LL << 30)) return 0;
  return ((size_t)L * L + (size_t)B * L * C) * sizeof(float);
}

int ffd_smooth_frequency(const float* x, float* out, void* work, size_t work_bytes, int B, int L, int C, double sigma,
                         void* stream) {
  if (!x || !out || !work || x == out) return FFD_ERR_INVALID;
  if (B < 1 || L < 1 || C < 1 || L % 2 == 0) return FFD_ERR_INVALID;  // even L: the reference's einsum raises
  if (!(sigma > 0.0) || !std::isfinite(sigma) || !((float)sigma > 0.f) || !std::isfinite((float)sigma)) return FFD_ERR_INVALID;
  const long long N = (long long)B * C;
  if (sp_check(B, L, C, SP_MAX_SMOOTH_L) != FFD_OK || N > (1LL << 30)) return FFD_ERR_UNSUPPORTED;
  if (work_bytes < ffd_smooth_frequency_work_bytes(B, L, C)) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  float* W = (float*)work;
  float* y = W + (size_t)L * L;
  if (int rc = ffd_dft(x, out, B, L, C, stream)) return rc;  // the spectrum waits in `out`
  hipLaunchKernelGGL(k_smooth_kernel, dim3(L), dim3(256), 0, s, W, L, (float)sigma);
  hipLaunchKernelGGL(k_smooth_mm, dim3(cdiv((int)N, 16)), dim3(256), 0, s, out, W, y, (int)N, L, C);
  if (hipGetLastError() != hipSuccess) return FFD_ERR_HIP;
  return ffd_idft(y, out, B, L, C, stream);
}

// doubles first (8-byte alignment of `work` is required): totals (B), slab partials, the plain means
static size_t prof_doubles(int B, int L) { return (size_t)B + (size_t)cdiv(B, PF_SLAB) * 2 * L + L; }

size_t ffd_spectral_profile_work_bytes(int B, int L, int C) {
  if (sp_check(B, L, C) != FFD_OK) return 0;
  return prof_doubles(B, L) * sizeof(double) + (sp_spec_floats(B, L, C) + (size_t)B * L) * sizeof(float);
}

int ffd_spectral_profile(const float* x, float* spec_mean, float* spec_se, float* energy_mean, float* energy_std,
                         void* work, size_t work_bytes, int B, int L, int C, void* stream) {
  if (!x || !spec_mean || !spec_se || !energy_mean || !energy_std || !work) return FFD_ERR_INVALID;
  if (int rc = sp_check(B, L, C)) return rc;
  if (work_bytes < ffd_spectral_profile_work_bytes(B, L, C) || ((uintptr_t)work & 7)) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int nf = L / 2 + 1;
  double* tot = (double*)work;
  double* part = tot + B;
  double* mean_p = part + (size_t)cdiv(B, PF_SLAB) * 2 * L;
  float* xf = (float*)(mean_p + L);
  float* dens = xf + (size_t)B * L * C;
  float* P = dens + (size_t)B * nf * C;
  if (int rc = sp_density(x, xf, dens, B, L, C, stream)) return rc;
  // spectral_interpretation.py:85-94: the temporal "SE" column is the plain std
  if (launch_norm_rows(x, B, L, C, 1, 0, P, tot, s) != hipSuccess) return FFD_ERR_HIP;
  if (launch_profile(P, tot, B, L, energy_mean, energy_std, 1.0, part, mean_p, s) != hipSuccess) return FFD_ERR_HIP;
  // spectral_interpretation.py:58-68: the un-mirrored density bins; SE = std / sqrt(B)
  if (launch_norm_rows(dens, B, nf, C, 0, 0, P, tot, s) != hipSuccess) return FFD_ERR_HIP;
  if (launch_profile(P, tot, B, nf, spec_mean, spec_se, 1.0 / sqrt((double)B), part, mean_p, s) != hipSuccess)
    return FFD_ERR_HIP;
  return FFD_OK;
}

// Benchmark helper (tools/spectral_bench.py; replaces nothing in the reference): ffd_localization's own stages
// (localization_stages) with HIP events between them, `warmup` untimed and `iters` timed runs.  x holds `n_inputs`
// consecutive (B, L, C) inputs and run i reads input i % n_inputs, so the caller decides whether the input can stay in
// the last-level cache.  ms_out[3 i + 0..2] = mean, minimum, maximum milliseconds of stage i: the time-domain rows,
// dft + density + frequency rows, the two product launches.  Synchronous.
int ffd_localization_bench(const float* x, int n_inputs, float* deloc_time_out, float* deloc_freq_out, void* work,
                           size_t work_bytes, int B, int L, int C, int warmup, int iters, float* ms_out, void* stream) {
  if (!x || !deloc_time_out || !deloc_freq_out || !work || !ms_out || n_inputs < 1 || warmup < 0 || iters < 1)
    return FFD_ERR_INVALID;
  if (int rc = sp_check(B, L, C)) return rc;
  if (work_bytes < ffd_localization_work_bytes(B, L, C)) return FFD_ERR_INVALID;
  struct Events {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() {
      for (hipEvent_t ev : e)
        if (ev) (void)hipEventDestroy(ev);
    }
  } ev;
  for (hipEvent_t& e : ev.e)
    if (hipEventCreate(&e) != hipSuccess) return FFD_ERR_HIP;
  double sum[3] = {0, 0, 0}, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {0, 0, 0};
  for (int it = -warmup; it < iters; ++it) {
    const float* xi = x + (size_t)((it + warmup) % n_inputs) * B * L * C;
    if (int rc = localization_stages(xi, deloc_time_out, deloc_freq_out, work, B, L, C, stream, ev.e)) return rc;
    if (hipEventSynchronize(ev.e[3]) != hipSuccess) return FFD_ERR_HIP;
    for (int i = 0; i < 3; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]) != hipSuccess) return FFD_ERR_HIP;
      if (it < 0) continue;
      sum[i] += ms;
      lo[i] = std::min(lo[i], (double)ms);
      hi[i] = std::max(hi[i], (double)ms);
    }
  }
  for (int i = 0; i < 3; ++i) {
    ms_out[3 * i] = (float)(sum[i] / iters);
    ms_out[3 * i + 1] = (float)lo[i];
    ms_out[3 * i + 2] = (float)hi[i];
  }
  return FFD_OK;
}

}  // extern "C"
