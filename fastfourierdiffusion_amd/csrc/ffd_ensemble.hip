// Scores of a forecast / imputation ensemble against the truth, on the device: CRPS, quantiles and ranks per point,
// the energy score per series (include/ffd.h ffd_ens_pointwise, ffd_ens_energy).  An ensemble is (S, m, D): S series,
// m members, D = L * C coordinates; a weight of 0 takes a coordinate (an observed one) out of every score.
//
// Per point.  The (m, D) slab of a series goes through the tiled transpose of the sample metrics (k_w2_columns) into
// rows of m keys, the rows through their segmented sort (k_w2_sort_chunk + k_w2_merge), and
//   k_ens_rows     reads one sorted row once: sum |x - y|, sum (2 i - m - 1) x_(i), the counts below / equal to y, the
//                  quantiles -- fp64, thread t takes i = t, t + 256, ..., then a fixed-order tree
//   k_ens_mean     crps_mean[s]: the mean of the row values over the coordinates with weight 1, the same way
// Rows (s, d) are cut into blocks by the workspace; a row's result depends on that row only.
//
// Energy score.  sum_ij ||x_i - x_j|| from the Gram matrix of the rows CENTRED on the series' ensemble mean: the
// uncentred n_i + n_j - 2 g_ij cancels for a tight ensemble far from the origin (offset 100, spread 1e-2: n is 1e6 D and
// d^2 is 1e-4 D, below fp32's resolution of n), centred rows are as large as the distances themselves.
//   k_ens_colpart + k_ens_colmean   the ensemble mean per coordinate (fp64 over fixed slabs of 1024 members, in order)
//   k_ens_centre   z = w (x - mean) into rows padded to a multiple of 16 columns, n_i = |z_i|^2, and the truth term
//                  ||x_i - y||_w in difference form (fp64)
//   k_ens_pairs    64 x 256 tiles of z z^T on the exact-fp32 16x16x4 MFMA (the operand scheme of k_w2_project: float4
//                  loads from the row-major rows, A and B sharing the k permutation), d^2 clamped at 0, sqrt, fp64 sum
//                  over j > i only (the fold doubles it; the diagonal never enters); a partial per workgroup
//   k_ens_energy   folds the partials and the truth terms in a fixed order
// The tiling depends on m alone, so a series' score does not depend on S, on the block cut or on the grid.
#include <algorithm>

#include "ffd_internal.h"

namespace ffd {

constexpr int ENS_MAX_Q = 64;
struct EnsLevels {
  double p[ENS_MAX_Q];
};

// ---- per point -------------------------------------------------------------------------------------------------
// One workgroup per row r = r0 + blockIdx.x = s D + d of the block; rows: (block rows, m) sorted ascending.
__global__ __launch_bounds__(256) void k_ens_rows(const float* __restrict__ rows, const float* __restrict__ truth,
                                                  const float* __restrict__ weight, int weight_stride, long long r0,
                                                  int m, int D, EnsLevels lv, int n_q, double z_norm,
                                                  double* __restrict__ crps, double* __restrict__ quant,
                                                  size_t quant_stride, int* __restrict__ below, int* __restrict__ equal) {
  __shared__ double red[256];
  const long long r = r0 + blockIdx.x;
  const long long s = r / D;
  const int d = (int)(r - s * D);
  const bool on = weight ? weight[(size_t)s * weight_stride + d] != 0.f : true;
  if (!on) {  // an observed coordinate: every output is 0
    if (threadIdx.x == 0) {
      if (crps) crps[r] = 0.0;
      if (below) below[r] = 0;
      if (equal) equal[r] = 0;
    }
    if (quant && (int)threadIdx.x < n_q) quant[(size_t)threadIdx.x * quant_stride + r] = 0.0;
    return;
  }
  const float* x = rows + (size_t)blockIdx.x * m;
  const float yf = truth[r];
  const double y = (double)yf;
  double sa = 0.0, sr = 0.0, nb = 0.0, ne = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) {
    const float v = x[i];
    sa += fabs((double)v - y);
    sr += (double)(2 * i + 1 - m) * (double)v;  // (2 i - m - 1) x_(i), i counted from 1: an exact product
    nb += v < yf ? 1.0 : 0.0;
    ne += v == yf ? 1.0 : 0.0;
  }
  sa = block_sum(sa, red);
  sr = block_sum(sr, red);
  nb = block_sum(nb, red);  // counts up to 2^20: exact in fp64
  ne = block_sum(ne, red);
  if (threadIdx.x == 0) {
    if (crps) crps[r] = sa / (double)m - sr / z_norm;
    if (below) below[r] = (int)nb;
    if (equal) equal[r] = (int)ne;
  }
  if (quant && (int)threadIdx.x < n_q) {
    // numpy's linear (type 7) quantile with its own interpolation: a + (b - a) g below g = 0.5, b - (b - a) (1 - g)
    // from there on; every operation rounded on its own, so the value is numpy's bit for bit
#pragma clang fp contract(off)
    const double h = (double)(m - 1) * lv.p[threadIdx.x];
    const double fl = floor(h);
    const double g = h - fl;
    const int lo = min((int)fl, m - 1), hi = min(lo + 1, m - 1);
    const double a = (double)x[lo], b = (double)x[hi];
    const double diff = b - a;
    double v = a + diff * g;
    if (g >= 0.5) v = b - diff * (1.0 - g);
    if (g == 0.0) v = a;  // levels 0 and 1: the minimum and the maximum themselves, also next to an infinity
    quant[(size_t)threadIdx.x * quant_stride + r] = v;
  }
}

// crps_mean[s] = the mean of crps[s, :] over the coordinates with weight 1 (0 where there is none)
__global__ __launch_bounds__(256) void k_ens_mean(const double* __restrict__ crps, const float* __restrict__ weight,
                                                  int weight_stride, int D, double* __restrict__ out) {
  __shared__ double red[256];
  const size_t s = blockIdx.x;
  double a = 0.0, n = 0.0;
  for (int d = threadIdx.x; d < D; d += 256) {
    const bool on = weight ? weight[s * weight_stride + d] != 0.f : true;
    a += on ? crps[s * D + d] : 0.0;
    n += on ? 1.0 : 0.0;
  }
  a = block_sum(a, red);
  n = block_sum(n, red);
  if (threadIdx.x == 0) out[s] = n > 0.0 ? a / n : 0.0;
}

// ---- energy score ----------------------------------------------------------------------------------------------
constexpr int ENS_SLAB = 1024;  // members per column-sum slab (fixed: the grid does not change the mean)
constexpr int EP_I = 64, EP_J = 256, EP_MAX_CHUNKS = 64;

// part[s][slab][d] = sum of x[s][i][d] over the slab's members, fp64, 4 member groups combined in order
__global__ __launch_bounds__(256) void k_ens_colpart(const float* __restrict__ X, int m, int D, int nslab,
                                                     double* __restrict__ part) {
  __shared__ double red[4][64];
  const int cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl, g = threadIdx.x >> 6;
  const size_t s = blockIdx.z;
  const int i0 = blockIdx.y * ENS_SLAB, i1 = min(i0 + ENS_SLAB, m);
  const float* xs = X + s * (size_t)m * D;
  double a = 0.0;
  if (c < D)
    for (int i = i0 + g; i < i1; i += 4) a += (double)xs[(size_t)i * D + c];
  red[g][cl] = a;
  __syncthreads();
  if (g == 0 && c < D) part[(s * nslab + blockIdx.y) * D + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}
__global__ __launch_bounds__(256) void k_ens_colmean(const double* __restrict__ part, int nslab, int m, int D,
                                                     float* __restrict__ mean, int mean_stride) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const size_t s = blockIdx.y;
  if (c >= D) return;
  double a = 0.0;
  for (int i = 0; i < nslab; ++i) a += part[(s * nslab + i) * D + c];
  mean[s * mean_stride + c] = (float)(a / (double)m);
}

__device__ __forceinline__ double wave_sum(double v) {  // a fixed butterfly: every lane gets the same total
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// A wave per member: z[i][d] = w_d (x[i][d] - mean[d]) (0 for D <= d < Dp), nrm[i] = |z_i|^2, tnorm[i] = ||x_i - y||_w
__global__ __launch_bounds__(256) void k_ens_centre(const float* __restrict__ X, const float* __restrict__ truth,
                                                    const float* __restrict__ weight, int weight_stride,
                                                    const float* __restrict__ mean, int mean_stride, float* __restrict__ Z,
                                                    float* __restrict__ nrm, double* __restrict__ tnorm, int m, int mp,
                                                    int D, int Dp) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const size_t s = blockIdx.y;
  if (i >= m) return;
  const float* x = X + (s * m + i) * (size_t)D;
  const float* y = truth + s * D;
  const float* w = weight ? weight + s * weight_stride : nullptr;
  const float* c = mean + s * mean_stride;
  float* z = Z + (s * m + i) * (size_t)Dp;
  double nn = 0.0, tt = 0.0;
  for (int d = lane; d < Dp; d += 64) {
    float zv = 0.f;
    if (d < D && (w ? w[d] != 0.f : true)) {
      const float xv = x[d];
      zv = xv - c[d];
      const double t = (double)xv - (double)y[d];
      tt += t * t;
    }
    z[d] = zv;
    nn += (double)zv * (double)zv;
  }
  nn = wave_sum(nn);
  tt = wave_sum(tt);
  if (lane == 0) {
    nrm[s * mp + i] = (float)nn;
    tnorm[s * mp + i] = sqrt(tt);
  }
}

// Workgroup (bi, ch) of series blockIdx.y: members i in [64 bi, 64 bi + 64) against the column tiles bj of chunk ch
// (CH tiles of 256 members) that reach past the diagonal; wave w owns members j in [64 w, 64 w + 64) of a tile as 4 x 4
// MFMA tiles.  A = z rows i, B = z rows j; lane group q = lane >> 4 holds k = 16 g + 4 q + {0..3} of both, MFMA step e
// pairs the e-th member of both.  Members past m are clamped for the loads and never counted.
__global__ __launch_bounds__(256) void k_ens_pairs(const float* __restrict__ Z, const float* __restrict__ nrm,
                                                   double* __restrict__ part, int m, int mp, int Dp, int nbj, int CH,
                                                   int nch, int npart) {
  __shared__ double red[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const size_t s = blockIdx.y;
  const int bi = blockIdx.x / nch, ch = blockIdx.x - bi * nch;
  const int i0 = bi * EP_I;
  const float* zs = Z + s * (size_t)m * Dp;
  const float* ns = nrm + s * mp;
  const int bj_lo = max(ch * CH, i0 / EP_J), bj_hi = min(ch * CH + CH, nbj);
  double total = 0.0;
  for (int bj = bj_lo; bj < bj_hi; ++bj) {
    const int j0 = bj * EP_J + wave * 64;
    if (j0 + 63 <= i0 || j0 >= m) continue;  // (wave-uniform) nothing of this wave's columns lies past the diagonal
    const float* ar[4];
    const float* br[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      ar[t] = zs + (size_t)min(i0 + 16 * t + c, m - 1) * Dp + 4 * q;
      br[t] = zs + (size_t)min(j0 + 16 * t + c, m - 1) * Dp + 4 * q;
    }
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < Dp; kb += 16) {
      f32x4 av[4], bv[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        av[t] = *(const f32x4*)(ar[t] + kb);
        bv[t] = *(const f32x4*)(br[t] + kb);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = mfma16(av[a][e], bv[b][e], acc[a][b]);
    }
    // D[i = 4 q + r][j = c]: member i0 + 16 a + 4 q + r against member j0 + 16 b + c
    float nj[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) nj[b] = ns[min(j0 + 16 * b + c, m - 1)];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * a + 4 * q + r;
        const float ni = ns[min(i, m - 1)];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int j = j0 + 16 * b + c;
          const float d2 = fmaxf((ni + nj[b]) - 2.f * acc[a][b][r], 0.f);
          if (j > i && j < m) total += (double)sqrtf(d2);
        }
      }
  }
  total = block_sum(total, red);
  if (threadIdx.x == 0) part[s * npart + blockIdx.x] = total;
}

// energy[s] = (1 / m) sum_i ||x_i - y||_w - (1 / Z) sum_{i < j} ||x_i - x_j||_w
__global__ __launch_bounds__(256) void k_ens_energy(const double* __restrict__ part, int npart, int npart_stride,
                                                    const double* __restrict__ tnorm, int m, int mp, double z_norm,
                                                    double* __restrict__ out) {
  __shared__ double red[256];
  const size_t s = blockIdx.x;
  double p = 0.0, t = 0.0;
  for (int i = threadIdx.x; i < npart; i += 256) p += part[s * npart_stride + i];
  for (int i = threadIdx.x; i < m; i += 256) t += tnorm[s * mp + i];
  p = block_sum(p, red);
  t = block_sum(t, red);
  if (threadIdx.x == 0) out[s] = t / (double)m - p / z_norm;
}

// ---- host: limits, workspace, blocks ---------------------------------------------------------------------------
constexpr int ENS_MAX_S = 1 << 20, ENS_MAX_M = 1 << 20, ENS_MAX_D = 1 << 20, ENS_MAX_BLOCK = 32768;

static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct EnergyPlan {
  int Dp, mp, nslab, nbi, nbj, CH, nch, npart, npart_stride;
  size_t colpart_doubles, series_bytes;
};
static EnergyPlan energy_plan(int m, int D) {
  EnergyPlan p;
  p.Dp = (int)up(D, 16);
  p.mp = (int)up(m, 4);
  p.nslab = cdiv(m, ENS_SLAB);
  p.nbi = cdiv(m, EP_I);
  p.nbj = cdiv(m, EP_J);
  p.CH = cdiv(p.nbj, EP_MAX_CHUNKS);
  p.nch = cdiv(p.nbj, p.CH);
  p.npart = p.nbi * p.nch;
  p.npart_stride = (int)up(p.npart, 2);
  p.colpart_doubles = up((size_t)p.nslab * D, 2);
  p.series_bytes = (size_t)m * p.Dp * 4 + 8 * ((size_t)p.mp + p.colpart_doubles + p.npart_stride) + 4 * ((size_t)p.mp + p.Dp);
  return p;
}
static size_t point_fixed_bytes(int S, int D) { return up((size_t)S * D * 8, 16); }

static int ens_check(int S, int m, int D, int fair, int weight_batch) {
  if (S < 1 || m < 1 || D < 1 || (fair && m < 2) || (weight_batch != 1 && weight_batch != S)) return FFD_ERR_INVALID;
  if (S > ENS_MAX_S || m > ENS_MAX_M || D > ENS_MAX_D) return FFD_ERR_UNSUPPORTED;
  return FFD_OK;
}
static double ens_z(int m, int fair) { return fair ? (double)m * (double)(m - 1) : (double)m * (double)m; }

struct EnsEvents {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  ~EnsEvents() {
    for (hipEvent_t ev : e)
      if (ev) (void)hipEventDestroy(ev);
  }
};

// One block of sb series (the pointers already at its first series).  stage 1: mean, centring, truth term; stage 2: the
// pair kernel; stage 4: the fold.
static hipError_t energy_block(int stages, const float* ens, const float* truth, const float* weight, int weight_stride,
                               int sb, int m, int D, const EnergyPlan& p, double z_norm, double* out, void* work,
                               hipStream_t s) {
  float* Z = (float*)work;
  double* tnorm = (double*)(Z + (size_t)sb * m * p.Dp);
  double* colpart = tnorm + (size_t)sb * p.mp;
  double* part = colpart + (size_t)sb * p.colpart_doubles;
  float* nrm = (float*)(part + (size_t)sb * p.npart_stride);
  float* mean = nrm + (size_t)sb * p.mp;
  if (stages & 1) {
    hipLaunchKernelGGL(k_ens_colpart, dim3(cdiv(D, 64), p.nslab, sb), dim3(256), 0, s, ens, m, D, p.nslab, colpart);
    hipLaunchKernelGGL(k_ens_colmean, dim3(cdiv(D, 256), sb), dim3(256), 0, s, colpart, p.nslab, m, D, mean, p.Dp);
    hipLaunchKernelGGL(k_ens_centre, dim3(cdiv(m, 4), sb), dim3(256), 0, s, ens, truth, weight, weight_stride, mean, p.Dp, Z,
                       nrm, tnorm, m, p.mp, D, p.Dp);
  }
  if (stages & 2)
    hipLaunchKernelGGL(k_ens_pairs, dim3(p.npart, sb), dim3(256), 0, s, Z, nrm, part, m, p.mp, p.Dp, p.nbj, p.CH, p.nch,
                       p.npart_stride);
  if (stages & 4)
    hipLaunchKernelGGL(k_ens_energy, dim3(sb), dim3(256), 0, s, part, p.npart, p.npart_stride, tnorm, m, p.mp, z_norm, out);
  return hipGetLastError();
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): the ensemble scores ----
using namespace ffd;

extern "C" {

size_t ffd_ens_work_bytes(int S, int m, int D, int n_q, size_t budget_bytes) {
  if (S < 1 || m < 1 || D < 1 || n_q < 0 || n_q > ENS_MAX_Q || S > ENS_MAX_S || m > ENS_MAX_M || D > ENS_MAX_D) return 0;
  const size_t fixed = point_fixed_bytes(S, D), row = 8 * (size_t)m;
  size_t rb = (budget_bytes > fixed ? budget_bytes - fixed : 0) / row;
  rb = std::max<size_t>(1, std::min<size_t>(rb, std::min<size_t>((size_t)S * D, ENS_MAX_BLOCK)));
  const size_t per = energy_plan(m, D).series_bytes;
  size_t sb = budget_bytes / per;
  sb = std::max<size_t>(1, std::min<size_t>(sb, (size_t)std::min(S, ENS_MAX_BLOCK)));
  return std::max(fixed + rb * row, sb * per);
}

int ffd_ens_pointwise(const float* ens, const float* truth, const float* weight, int weight_batch, int S, int m, int D,
                      const double* levels, int n_q, int fair, double* crps_out, double* crps_mean_out, double* quant_out,
                      int* below_out, int* equal_out, void* work, size_t work_bytes, void* stream) {
  if (!ens || !truth || !work || n_q < 0 || n_q > ENS_MAX_Q || (quant_out && n_q > 0 && !levels)) return FFD_ERR_INVALID;
  if (int rc = ens_check(S, m, D, fair, weight ? weight_batch : 1)) return rc;
  EnsLevels lv = {};
  if (quant_out)
    for (int i = 0; i < n_q; ++i) {
      if (!(levels[i] >= 0.0 && levels[i] <= 1.0)) return FFD_ERR_INVALID;
      lv.p[i] = levels[i];
    }
  const size_t fixed = point_fixed_bytes(S, D), row = 8 * (size_t)m;
  if (((uintptr_t)work & 15) || work_bytes < fixed + row) return FFD_ERR_INVALID;
  const long long R = (long long)S * D;
  const long long Rb = (long long)std::min<size_t>((work_bytes - fixed) / row, (size_t)std::min<long long>(R, ENS_MAX_BLOCK));
  hipStream_t s = (hipStream_t)stream;
  double* crps = crps_out ? crps_out : (crps_mean_out ? (double*)work : nullptr);
  float* rows = (float*)((char*)work + fixed);
  float* scratch = rows + (size_t)Rb * m;
  const int wstride = weight && weight_batch == S && S > 1 ? D : 0;
  double* quant = quant_out && n_q > 0 ? quant_out : nullptr;
  for (long long r0 = 0; r0 < R; r0 += Rb) {
    const long long rb = std::min(Rb, R - r0);
    for (long long r = r0; r < r0 + rb;) {  // the series this block meets: their columns, transposed into its rows
      const long long sr = r / D;
      const int d0 = (int)(r - sr * D), nc = (int)std::min<long long>(D - d0, r0 + rb - r);
      if (launch_w2_columns(ens + (size_t)sr * m * D, rows + (size_t)(r - r0) * m, m, D, d0, nc, s) != hipSuccess)
        return FFD_ERR_HIP;
      r += nc;
    }
    if (launch_w2_sort(rows, scratch, m, (int)rb, s) != hipSuccess) return FFD_ERR_HIP;
    hipLaunchKernelGGL(k_ens_rows, dim3((unsigned)rb), dim3(256), 0, s, rows, truth, weight, wstride, r0, m, D, lv, n_q,
                       ens_z(m, fair), crps, quant, (size_t)R, below_out, equal_out);
    if (hipGetLastError() != hipSuccess) return FFD_ERR_HIP;
  }
  if (crps_mean_out) {
    hipLaunchKernelGGL(k_ens_mean, dim3(S), dim3(256), 0, s, crps, weight, wstride, D, crps_mean_out);
    if (hipGetLastError() != hipSuccess) return FFD_ERR_HIP;
  }
  return FFD_OK;
}

static int ens_energy_args(const float* ens, const float* truth, const float* weight, int weight_batch, int S, int m, int D,
                           int fair, const double* energy_out, const void* work, size_t work_bytes, int* sb_out) {
  if (!ens || !truth || !energy_out || !work) return FFD_ERR_INVALID;
  if (int rc = ens_check(S, m, D, fair, weight ? weight_batch : 1)) return rc;
  const size_t per = energy_plan(m, D).series_bytes;
  if (((uintptr_t)work & 15) || work_bytes < per) return FFD_ERR_INVALID;
  *sb_out = (int)std::min<size_t>(work_bytes / per, (size_t)std::min(S, ENS_MAX_BLOCK));
  return FFD_OK;
}

int ffd_ens_energy(const float* ens, const float* truth, const float* weight, int weight_batch, int S, int m, int D, int fair,
                   double* energy_out, void* work, size_t work_bytes, void* stream) {
  int Sb = 0;
  if (int rc = ens_energy_args(ens, truth, weight, weight_batch, S, m, D, fair, energy_out, work, work_bytes, &Sb)) return rc;
  const EnergyPlan p = energy_plan(m, D);
  const int wstride = weight && weight_batch == S && S > 1 ? D : 0;
  for (int s0 = 0; s0 < S; s0 += Sb) {
    const int sb = std::min(Sb, S - s0);
    if (energy_block(7, ens + (size_t)s0 * m * D, truth + (size_t)s0 * D, weight ? weight + (size_t)s0 * wstride : nullptr,
                     wstride, sb, m, D, p, ens_z(m, fair), energy_out + s0, work, (hipStream_t)stream) != hipSuccess)
      return FFD_ERR_HIP;
  }
  return FFD_OK;
}

// Benchmark helper (tools/ensemble_bench.py): ffd_ens_energy's stages with HIP events between them.
int ffd_ens_bench_energy(const float* ens, const float* truth, const float* weight, int weight_batch, int S, int m, int D,
                         int fair, double* energy_out, void* work, size_t work_bytes, int iters, float* ms_out,
                         void* stream) {
  int Sb = 0;
  if (!ms_out || iters < 1) return FFD_ERR_INVALID;
  if (int rc = ens_energy_args(ens, truth, weight, weight_batch, S, m, D, fair, energy_out, work, work_bytes, &Sb)) return rc;
  if (Sb < S) return FFD_ERR_INVALID;  // one block: the stages of different blocks would share the workspace
  const EnergyPlan p = energy_plan(m, D);
  const int wstride = weight && weight_batch == S && S > 1 ? D : 0;
  hipStream_t s = (hipStream_t)stream;
  EnsEvents ev;
  for (hipEvent_t& e : ev.e)
    if (hipEventCreate(&e) != hipSuccess) return FFD_ERR_HIP;
  double acc[2] = {0, 0};
  for (int it = -1; it < iters; ++it) {  // iteration -1 warms up
    float a = 0.f, b = 0.f;
    const bool ok = hipEventRecord(ev.e[0], s) == hipSuccess &&
                    energy_block(1, ens, truth, weight, wstride, S, m, D, p, ens_z(m, fair), energy_out, work, s) == hipSuccess &&
                    hipEventRecord(ev.e[1], s) == hipSuccess &&
                    energy_block(2, ens, truth, weight, wstride, S, m, D, p, ens_z(m, fair), energy_out, work, s) == hipSuccess &&
                    hipEventRecord(ev.e[2], s) == hipSuccess &&
                    energy_block(4, ens, truth, weight, wstride, S, m, D, p, ens_z(m, fair), energy_out, work, s) == hipSuccess &&
                    hipEventSynchronize(ev.e[2]) == hipSuccess && hipEventElapsedTime(&a, ev.e[0], ev.e[1]) == hipSuccess &&
                    hipEventElapsedTime(&b, ev.e[1], ev.e[2]) == hipSuccess;
    if (!ok) return FFD_ERR_HIP;
    if (it >= 0) {
      acc[0] += a;
      acc[1] += b;
    }
  }
  ms_out[0] = (float)(acc[0] / iters);
  ms_out[1] = (float)(acc[1] / iters);
  return FFD_OK;
}

}  // extern "C"
