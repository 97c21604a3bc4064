// Kernel two-sample statistics between two row sets, on the device: Gaussian-kernel row sums, the unbiased and biased
// maximum mean discrepancy, per-sample witness values, a closed-form bandwidth, and a permutation test (include/ffd.h
// ffd_mmd_*).  Rows are flat fp32 vectors (n, D); k_gamma(a, b) = exp(-gamma |a - b|^2), up to 8 gammas per call.
//
// The pair tile is the nearest-neighbour one (ffd_pairtile.h): both sets centred on ONE caller-supplied vector, the
// exact-fp32 16x16x4 MFMA Gram form in 64 x 256 tiles, nn_d2.  No distance or kernel block goes through memory for the
// row sums: the epilogue is an exponential and a sum.  Rows of more than 1024 padded columns take the tile's sum over k in
// chunks of 1024 through LDS (nn_tile's spill): one fp32 chain over 65 536 terms misses the bar on kernel values, which
// see the error of d^2 times gamma; up to 1024 columns nothing changes.
//   k_mmd_rowsums  a workgroup owns 64 query rows and walks a run of MMD_RUN column tiles in order; a lane adds its
//                  kernel values (fp32, one v_exp_f32 per gamma) to fp64 sums in (tile, b, r) order, the four lane
//                  groups and the four waves are combined in a fixed order: part[run][g][i]
//   k_mmd_fold     folds the runs' partial sums in run order
//                  => a row's sum depends on its row, the column set and the centre alone: the same bits from run to
//                  run, for a query set summed whole or in parts, whatever rows surround it
//   k_mmd_sqdev + k_mmd_sigma2   sigma^2 = 2 n / (n - 1) mean |y - ybar|^2, all fp64 (ybar: k_nn_colpart + k_nn_colmean)
//   k_mmd_scores + k_mmd_witness MMD^2 (unbiased, biased) per gamma and for the mean kernel, w_i; fixed-order fp64 trees
//   k_mmd_gram     the pooled mean-kernel matrix K (N x N, diagonal 0, row stride a multiple of 64) into the workspace
//   k_mmd_assign + k_mmd_krowsum + k_mmd_perm + k_mmd_perm_fold   T_p for P assignments: S = K A^T on the fp64 matrix
//                  instruction (v_mfma_f64_16x16x4_f64; K's fp32 entries and the 0 / 1 assignments are exact in fp64, so
//                  the accumulation carries fp64 rounding only and K needs no centring), reduced per 64-row block to
//                  (a^T K a, b^T K a, b^T K b) and folded in block order
// The one-bandwidth-per-exponential epilogue is the only one: a doubling ladder is NOT taken from the narrowest
// exponent by squaring, so n_gamma gammas in one call give the bits of n_gamma calls.
// Diagonal tiles of the self terms are computed in full (no use of symmetry).  No atomics anywhere.
#include <algorithm>
#include <cmath>

#include "ffd_pairtile.h"

namespace ffd {

constexpr int MMD_RUN = 4;  // column tiles (of 256) one workgroup walks: a constant of the source, never of the grid
constexpr int MMD_MAX_G = FFD_MMD_MAX_GAMMAS;
struct MmdGammas {
  float c[MMD_MAX_G];  // -gamma log2(e), rounded once
};

// ---- row sums ------------------------------------------------------------------------------------------------------
// Workgroup (blockIdx.x = 64-row block, blockIdx.y = run): part[run][g][i] = sum over the run's columns of k_g(a_i, b_j)
template <int NG>
__global__ __launch_bounds__(256) void k_mmd_rowsums(const float* __restrict__ Za, const float* __restrict__ na_nrm, int na,
                                                     const float* __restrict__ Zb, const float* __restrict__ nb_nrm, int nb,
                                                     int Dp, MmdGammas gm, int exclude_self, int nbj,
                                                     double* __restrict__ part) {
  __shared__ double red[4][64];
  extern __shared__ __align__(16) float mmd_spill[];  // NN_SPILL_BYTES where Dp > NN_K_CHUNK, else none
  float* spill = Dp > NN_K_CHUNK ? mmd_spill : nullptr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int i0 = blockIdx.x * NN_I, run = blockIdx.y;
  float ni[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) ni[a] = na_nrm[min(i0 + 16 * a + c, na - 1)];
  double sum[NG][4];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int a = 0; a < 4; ++a) sum[g][a] = 0.0;
  const int bj_hi = min(run * MMD_RUN + MMD_RUN, nbj);
  for (int bj = run * MMD_RUN; bj < bj_hi; ++bj) {
    const int j0 = bj * NN_J + wave * 64;
    if (j0 >= nb) continue;  // (wave-uniform)
    f32x4 acc[4][4];
    nn_tile(Za, na, i0, Zb, nb, j0, Dp, q, c, acc, spill);
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 16 * b + 4 * q + r;
        const float nj = nb_nrm[min(j, nb - 1)];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int i = i0 + 16 * a + c;
          const bool in = j < nb && !(exclude_self && i == j);  // the pair i == j is never formed and subtracted
          const float d2 = nn_d2(ni[a], nj, acc[a][b][r]);
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            const float kv = __builtin_amdgcn_exp2f(d2 * gm.c[g]);
            sum[g][a] += in ? (double)kv : 0.0;
          }
        }
      }
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double v = sum[g][a];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (q == 0) red[wave][16 * a + c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      const int i = i0 + (int)threadIdx.x;
      if (i < na)
        part[((size_t)run * NG + g) * na + i] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
    __syncthreads();
  }
}

// out[x] = sum over the runs, in run order, of part[run][x]; x over (gamma, row)
__global__ __launch_bounds__(256) void k_mmd_fold(const double* __restrict__ part, int nruns, size_t total,
                                                  double* __restrict__ out) {
  const size_t x = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= total) return;
  double a = 0.0;
  for (int r = 0; r < nruns; ++r) a += part[(size_t)r * total + x];
  out[x] = a;
}

// ---- bandwidth -----------------------------------------------------------------------------------------------------
// A wave per row: dev[i] = sum_d ((double)y[i][d] - mean[d])^2, lane l takes d = l, l + 64, ..., then the butterfly
__global__ __launch_bounds__(256) void k_mmd_sqdev(const float* __restrict__ Y, const double* __restrict__ mean, int n, int D,
                                                   double* __restrict__ dev) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* y = Y + (size_t)i * D;
  double s = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double t = (double)y[d] - mean[d];
    s += t * t;
  }
  s = nn_wave_sum(s);
  if (lane == 0) dev[i] = s;
}
// One workgroup: sigma^2 = 2 (n / (n - 1)) (sum dev / n)
__global__ __launch_bounds__(256) void k_mmd_sigma2(const double* __restrict__ dev, int n, double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += dev[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = 2.0 * ((double)n / (double)(n - 1)) * (s / (double)n);
}

// ---- scores --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double mmd_strided_sum(const double* v, int n, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  return block_sum(s, red);
}
__device__ __forceinline__ double mmd_unbiased(double sxx, double sxy, double syy, double n, double m) {
  return (sxx / (n * (n - 1.0)) + syy / (m * (m - 1.0))) - 2.0 * sxy / (n * m);
}
__device__ __forceinline__ double mmd_biased(double sxx, double sxy, double syy, double n, double m) {
  return ((sxx + n) / (n * n) + (syy + m) / (m * m)) - 2.0 * sxy / (n * m);  // the diagonal: exactly 1 per row
}
// One workgroup.  out (2, ng + 1): row 0 unbiased, row 1 biased; column g < ng that gamma, column ng the mean kernel
__global__ __launch_bounds__(256) void k_mmd_scores(const double* __restrict__ xx, const double* __restrict__ xy,
                                                    const double* __restrict__ yy, int n, int m, int ng,
                                                    double* __restrict__ out) {
  __shared__ double red[256];
  double txx = 0.0, txy = 0.0, tyy = 0.0;
  for (int g = 0; g < ng; ++g) {
    const double sxx = mmd_strided_sum(xx + (size_t)g * n, n, red);
    const double sxy = mmd_strided_sum(xy + (size_t)g * n, n, red);
    const double syy = mmd_strided_sum(yy + (size_t)g * m, m, red);
    if (threadIdx.x == 0) {
      out[g] = mmd_unbiased(sxx, sxy, syy, n, m);
      out[ng + 1 + g] = mmd_biased(sxx, sxy, syy, n, m);
    }
    txx += sxx, txy += sxy, tyy += syy;
  }
  if (threadIdx.x == 0) {
    const double k = (double)ng;
    out[ng] = mmd_unbiased(txx / k, txy / k, tyy / k, n, m);
    out[2 * ng + 1] = mmd_biased(txx / k, txy / k, tyy / k, n, m);
  }
}
// w[i] = (mean_g xx[g][i]) / (n - 1) - (mean_g xy[g][i]) / m
__global__ __launch_bounds__(256) void k_mmd_witness(const double* __restrict__ xx, const double* __restrict__ xy, int n, int m,
                                                     int ng, double* __restrict__ w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double a = 0.0, b = 0.0;
  for (int g = 0; g < ng; ++g) {
    a += xx[(size_t)g * n + i];
    b += xy[(size_t)g * n + i];
  }
  w[i] = (a / (double)ng) / (double)(n - 1) - (b / (double)ng) / (double)m;
}

// ---- permutation test ----------------------------------------------------------------------------------------------
// Workgroup blockIdx.x = bi * nbj + bj: rows [64 bi, + 64) x columns [256 bj, + 256) of K, wave w 64 of the columns.
// K[i][j] = (1 / ng) sum_g k_g(z_i, z_j) for i != j < N, 0 on the diagonal and in the padding columns N <= j < Np.
__global__ __launch_bounds__(256) void k_mmd_gram(const float* __restrict__ Z, const float* __restrict__ nrm, int N, int Dp,
                                                  MmdGammas gm, int ng, float inv_ng, int nbj, float* __restrict__ K,
                                                  int Np) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int bi = blockIdx.x / nbj, bj = blockIdx.x - bi * nbj;
  const int i0 = bi * NN_I, j0 = bj * NN_J + wave * 64;
  if (j0 >= Np) return;  // (wave-uniform; Np is a multiple of 64: the 64 columns from j0 lie inside a row)
  extern __shared__ __align__(16) float mmd_spill[];  // NN_SPILL_BYTES where Dp > NN_K_CHUNK, else none
  f32x4 acc[4][4];
  nn_tile(Z, N, i0, Z, N, j0, Dp, q, c, acc, Dp > NN_K_CHUNK ? mmd_spill : nullptr);
  float nj[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) nj[b][r] = nrm[min(j0 + 16 * b + 4 * q + r, N - 1)];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + 16 * a + c;
    if (i >= N) continue;
    const float ni = nrm[i];
    float* krow = K + (size_t)i * Np + j0 + 4 * q;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 16 * b + 4 * q + r;
        const float d2 = nn_d2(ni, nj[b][r], acc[a][b][r]);
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < MMD_MAX_G; ++g)
          if (g < ng) s += __builtin_amdgcn_exp2f(d2 * gm.c[g]);  // (wave-uniform)
        o[r] = (j < N && j != i) ? s * inv_ng : 0.f;
      }
      *(f32x4*)(krow + 16 * b) = o;
    }
  }
}

// Ap (Pp, Np) bytes: the assignments as 0 / 1 with zero rows and columns of padding
__global__ __launch_bounds__(256) void k_mmd_assign(const uint8_t* __restrict__ A, int P, int N, uint8_t* __restrict__ Ap,
                                                    int Pp, int Np) {
  const size_t x = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= (size_t)Pp * Np) return;
  const int p = (int)(x / Np), k = (int)(x - (size_t)p * Np);
  Ap[x] = (p < P && k < N && A[(size_t)p * N + k] != 0) ? 1 : 0;
}
// A wave per row: rowtot[i] = sum_j K[i][j], fp64
__global__ __launch_bounds__(256) void k_mmd_krowsum(const float* __restrict__ K, int N, int Np, double* __restrict__ rowtot) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  double s = 0.0;
  for (int j = lane; j < N; j += 64) s += (double)K[(size_t)i * Np + j];
  s = nn_wave_sum(s);
  if (lane == 0) rowtot[i] = s;
}

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Workgroup (blockIdx.x = 64-row block ib of K, blockIdx.y = 256 assignments), wave w 64 of the assignments.
// s[i][p] = sum_k K[i][k] a_p[k] on v_mfma_f64_16x16x4_f64 (A operand: lane holds K[i = lane & 15][k = lane >> 4]; B:
// a_p[k = lane >> 4] of p = lane & 15; D register r of a lane: row (lane >> 4) + 4 r, column lane & 15).  Lane group q
// loads k = kb + 4 q + {0..3} of both operands and step e pairs the e-th of both.  Then per assignment, over the block's
// rows i < N:  u = sum_{i in a} s,  v = sum_{i not in a} s,  w = sum_{i not in a} (rowtot_i - s):  part[ib][3][Pp].
__global__ __launch_bounds__(256) void k_mmd_perm(const float* __restrict__ K, int N, int Np, const uint8_t* __restrict__ Ap,
                                                  int Pp, const double* __restrict__ rowtot, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int ib = blockIdx.x, i0 = ib * 64, p0 = (blockIdx.y * 4 + wave) * 64;
  if (p0 >= Pp) return;  // (wave-uniform)
  const float* kr[4];
  const uint8_t* pr[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    kr[t] = K + (size_t)min(i0 + 16 * t + c, N - 1) * Np + 4 * q;
    pr[t] = Ap + (size_t)(p0 + 16 * t + c) * Np + 4 * q;
  }
  f64x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int kb = 0; kb < Np; kb += 16) {
    f32x4 kv[4];
    uint32_t pv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      kv[t] = *(const f32x4*)(kr[t] + kb);
      pv[t] = *(const uint32_t*)(pr[t] + kb);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double ka[4], pa[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        ka[t] = (double)kv[t][e];
        pa[t] = (double)((pv[t] >> (8 * e)) & 1u);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ka[a], pa[b], acc[a][b], 0, 0, 0);
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int p = p0 + 16 * b + c;
    const uint8_t* arow = Ap + (size_t)p * Np;
    double u = 0.0, v = 0.0, w = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * a + q + 4 * r;
        if (i < N) {
          const double s = acc[a][b][r];
          if (arow[i]) {
            u += s;
          } else {
            v += s;
            w += rowtot[i] - s;
          }
        }
      }
    u += __shfl_xor(u, 16, 64), v += __shfl_xor(v, 16, 64), w += __shfl_xor(w, 16, 64);
    u += __shfl_xor(u, 32, 64), v += __shfl_xor(v, 32, 64), w += __shfl_xor(w, 32, 64);
    if (q == 0) {
      double* o = part + (size_t)ib * 3 * Pp + p;
      o[0] = u, o[Pp] = v, o[2 * (size_t)Pp] = w;
    }
  }
}
// T_p = u / (n (n - 1)) + w / (m (m - 1)) - 2 v / (n m), the blocks' parts added in block order
__global__ __launch_bounds__(256) void k_mmd_perm_fold(const double* __restrict__ part, int nib, int Pp, int P, int n, int m,
                                                       double* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  double u = 0.0, v = 0.0, w = 0.0;
  for (int ib = 0; ib < nib; ++ib) {
    const double* o = part + (size_t)ib * 3 * Pp + p;
    u += o[0], v += o[Pp], w += o[2 * (size_t)Pp];
  }
  const double dn = (double)n, dm = (double)m;
  out[p] = (u / (dn * (dn - 1.0)) + w / (dm * (dm - 1.0))) - 2.0 * v / (dn * dm);
}

// ---- host: checks, workspaces --------------------------------------------------------------------------------------
// FFD_OK and the rounded exponents, or FFD_ERR_INVALID: gammas finite, >= 0, -gamma log2(e) finite in fp32
static int mmd_gammas(const double* gammas, int n_gamma, MmdGammas* out) {
  if (!gammas || n_gamma < 1 || n_gamma > MMD_MAX_G) return FFD_ERR_INVALID;
  for (int g = 0; g < MMD_MAX_G; ++g) out->c[g] = 0.f;
  for (int g = 0; g < n_gamma; ++g) {
    if (!std::isfinite(gammas[g]) || gammas[g] < 0.0) return FFD_ERR_INVALID;
    const float c = (float)(-gammas[g] * 1.4426950408889634);
    if (!std::isfinite(c)) return FFD_ERR_INVALID;
    out->c[g] = c;
  }
  return FFD_OK;
}

// The row sums' workspace: the centred pair (b the reference, a the query side) and the runs' partial sums
struct MmdRowPlan {
  PairPlan pair;
  int nbi, nbj, nruns;
  size_t part, bytes;
};
static MmdRowPlan mmd_row_plan(int na, int nb, int D, int n_gamma) {
  MmdRowPlan p;
  p.nbi = cdiv(na, NN_I);
  p.nbj = cdiv(nb, NN_J);
  p.nruns = cdiv(p.nbj, MMD_RUN);
  Carver c;
  p.pair = nn_pair_plan(c, na, nb, D);
  p.part = c.take((size_t)p.nruns * n_gamma * na * 8);
  p.bytes = c.total;
  return p;
}

template <int NG>
static void mmd_launch_rowsums(const MmdRowPlan& p, const float* Za, const float* nrm_a, int na, const float* Zb,
                               const float* nrm_b, int nb, const MmdGammas& gm, int exclude_self, double* part,
                               hipStream_t s) {
  const size_t lds = nn_spill_bytes(k_mmd_rowsums<NG>, p.pair.Dp);
  hipLaunchKernelGGL(k_mmd_rowsums<NG>, dim3(p.nbi, p.nruns), dim3(256), lds, s, Za, nrm_a, na, Zb, nrm_b, nb, p.pair.Dp,
                     gm, exclude_self, p.nbj, part);
}

struct MmdGramPlan {
  int N, Np, Dp;
  size_t k, z, nrm, bytes;
};
static MmdGramPlan mmd_gram_plan(int n, int m, int D) {
  MmdGramPlan p;
  p.N = n + m;
  p.Np = (int)nn_up(p.N, 64);
  p.Dp = (int)nn_up(D, 16);
  Carver c;
  p.k = c.take((size_t)p.N * p.Np * 4);
  p.z = c.take((size_t)p.N * p.Dp * 4);
  p.nrm = c.take((size_t)p.N * 4);
  p.bytes = c.total;
  return p;
}
struct MmdPermPlan {
  int N, Np, Pp, nib;
  size_t ap, rowtot, part, bytes;
};
static MmdPermPlan mmd_perm_plan(int n, int m, int P) {
  MmdPermPlan p;
  p.N = n + m;
  p.Np = (int)nn_up(p.N, 64);
  p.Pp = (int)nn_up(P, 64);
  p.nib = cdiv(p.N, 64);
  Carver c;
  p.ap = c.take((size_t)p.Pp * p.Np);
  p.rowtot = c.take((size_t)p.N * 8);
  p.part = c.take((size_t)p.nib * 3 * p.Pp * 8);
  p.bytes = c.total;
  return p;
}
// The bandwidth's workspace: the slab sums, the fp64 mean, every row's squared deviation
struct MmdBandPlan {
  size_t colpart, mean, dev, bytes;
};
static MmdBandPlan mmd_band_plan(int n, int D) {
  MmdBandPlan p;
  Carver c;
  p.colpart = c.take(nn_colpart_bytes(n, D));
  p.mean = c.take((size_t)D * 8);
  p.dev = c.take((size_t)n * 8);
  p.bytes = c.total;
  return p;
}
static bool mmd_pool_ok(int n, int m) { return n >= 2 && m >= 2; }
static bool mmd_pool_supported(int n, int m) { return (long long)n + (long long)m <= FFD_MMD_MAX_POOLED; }

}  // namespace ffd

// ---- C ABI (include/ffd.h): kernel two-sample statistics ----
using namespace ffd;

extern "C" {

size_t ffd_mmd_centre_work_bytes(int n, int D) {
  if (!nn_shape_ok(n, n, D) || !nn_shape_supported(n, n, D)) return 0;
  return nn_up(nn_colpart_bytes(n, D), 16);
}

int ffd_mmd_centre(const float* x, int n, int D, float* centre_out, void* work, size_t work_bytes, void* stream) {
  if (!x || !centre_out || !work || !nn_shape_ok(n, n, D)) return FFD_ERR_INVALID;
  if (!nn_shape_supported(n, n, D)) return FFD_ERR_UNSUPPORTED;
  if (!work_ok(work, work_bytes, ffd_mmd_centre_work_bytes(n, D))) return FFD_ERR_INVALID;
  if (regions_clash({{centre_out, (size_t)D * 4}, {work, work_bytes}}, {{x, (size_t)n * D * 4}})) return FFD_ERR_INVALID;
  nn_launch_colmean(x, n, D, (double*)work, centre_out, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_mmd_bandwidth_work_bytes(int n, int D) {
  if (n < 2 || !nn_shape_ok(n, n, D) || !nn_shape_supported(n, n, D)) return 0;
  return mmd_band_plan(n, D).bytes;
}

int ffd_mmd_bandwidth(const float* y, int n, int D, double* sigma2_out, void* work, size_t work_bytes, void* stream) {
  if (!y || !sigma2_out || !work || n < 2 || !nn_shape_ok(n, n, D)) return FFD_ERR_INVALID;
  if (!nn_shape_supported(n, n, D)) return FFD_ERR_UNSUPPORTED;
  const MmdBandPlan p = mmd_band_plan(n, D);
  if (!work_ok(work, work_bytes, p.bytes)) return FFD_ERR_INVALID;
  if (regions_clash({{sigma2_out, 8}, {work, work_bytes}}, {{y, (size_t)n * D * 4}})) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  double* mean = (double*)(w + p.mean);
  double* dev = (double*)(w + p.dev);
  nn_launch_colmean(y, n, D, (double*)(w + p.colpart), mean, s);
  hipLaunchKernelGGL(k_mmd_sqdev, dim3(cdiv(n, 4)), dim3(256), 0, s, y, mean, n, D, dev);
  hipLaunchKernelGGL(k_mmd_sigma2, dim3(1), dim3(256), 0, s, dev, n, sigma2_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_mmd_rowsums_work_bytes(int na, int nb, int D, int n_gamma) {
  if (!nn_shape_ok(na, nb, D) || !nn_shape_supported(na, nb, D) || n_gamma < 1 || n_gamma > MMD_MAX_G) return 0;
  return mmd_row_plan(na, nb, D, n_gamma).bytes;
}

int ffd_mmd_rowsums(const float* a, int na, const float* b, int nb, int D, const float* centre, const double* gammas,
                    int n_gamma, int exclude_self, double* rowsum_out, void* work, size_t work_bytes, void* stream) {
  if (!a || !b || !centre || !rowsum_out || !work || !nn_shape_ok(na, nb, D)) return FFD_ERR_INVALID;
  MmdGammas gm;
  if (mmd_gammas(gammas, n_gamma, &gm) != FFD_OK) return FFD_ERR_INVALID;
  if (exclude_self && (a != b || na != nb)) return FFD_ERR_INVALID;
  if (!nn_shape_supported(na, nb, D)) return FFD_ERR_UNSUPPORTED;
  const MmdRowPlan p = mmd_row_plan(na, nb, D, n_gamma);
  if (!work_ok(work, work_bytes, p.bytes)) return FFD_ERR_INVALID;
  const size_t ab = (size_t)na * D * 4, bb = (size_t)nb * D * 4, cb = (size_t)D * 4, ob = (size_t)n_gamma * na * 8;
  if (regions_clash({{rowsum_out, ob}, {work, work_bytes}}, {{a, ab}, {b, bb}, {centre, cb}})) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  const PairRows z = nn_centre_pair(a, na, b, nb, D, centre, p.pair, w, s);
  double* part = (double*)(w + p.part);
  const int ex = exclude_self ? 1 : 0;
  switch (n_gamma) {
#define FFD_MMD_CASE(NG) \
  case NG: mmd_launch_rowsums<NG>(p, z.Zq, z.nrm_q, na, z.Zr, z.nrm_r, nb, gm, ex, part, s); break;
    FFD_MMD_CASE(1) FFD_MMD_CASE(2) FFD_MMD_CASE(3) FFD_MMD_CASE(4) FFD_MMD_CASE(5) FFD_MMD_CASE(6) FFD_MMD_CASE(7)
    FFD_MMD_CASE(8)
#undef FFD_MMD_CASE
  }
  const size_t total = (size_t)n_gamma * na;
  hipLaunchKernelGGL(k_mmd_fold, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, p.nruns, total, rowsum_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_mmd_scores(const double* rowsum_xx, const double* rowsum_xy, const double* rowsum_yy, int n, int m, int n_gamma,
                   double* mmd2_out, double* witness_out, void* stream) {
  if (!rowsum_xx || !rowsum_xy || !rowsum_yy || !mmd2_out || !witness_out) return FFD_ERR_INVALID;
  if (n < 2 || m < 2 || n_gamma < 1 || n_gamma > MMD_MAX_G) return FFD_ERR_INVALID;
  if (n > NN_MAX_ROWS || m > NN_MAX_ROWS) return FFD_ERR_UNSUPPORTED;
  const size_t xb = (size_t)n_gamma * n * 8, yb = (size_t)n_gamma * m * 8, ob = (size_t)(2 * n_gamma + 2) * 8,
               wb = (size_t)n * 8;
  if (regions_clash({{mmd2_out, ob}, {witness_out, wb}}, {{rowsum_xx, xb}, {rowsum_xy, xb}, {rowsum_yy, yb}}))
    return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mmd_scores, dim3(1), dim3(256), 0, s, rowsum_xx, rowsum_xy, rowsum_yy, n, m, n_gamma, mmd2_out);
  hipLaunchKernelGGL(k_mmd_witness, dim3(cdiv(n, 256)), dim3(256), 0, s, rowsum_xx, rowsum_xy, n, m, n_gamma, witness_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_mmd_gram_work_bytes(int n, int m, int D) {
  if (!mmd_pool_ok(n, m) || D < 1 || !mmd_pool_supported(n, m) || D > NN_MAX_D) return 0;
  return mmd_gram_plan(n, m, D).bytes;
}

int ffd_mmd_gram(const float* x, int n, const float* y, int m, int D, const float* centre, const double* gammas, int n_gamma,
                 void* work, size_t work_bytes, void* stream) {
  if (!x || !y || !centre || !work || !mmd_pool_ok(n, m) || D < 1) return FFD_ERR_INVALID;
  MmdGammas gm;
  if (mmd_gammas(gammas, n_gamma, &gm) != FFD_OK) return FFD_ERR_INVALID;
  if (!mmd_pool_supported(n, m) || D > NN_MAX_D) return FFD_ERR_UNSUPPORTED;
  const MmdGramPlan p = mmd_gram_plan(n, m, D);
  if (!work_ok(work, work_bytes, p.bytes)) return FFD_ERR_INVALID;
  const size_t xb = (size_t)n * D * 4, yb = (size_t)m * D * 4, cb = (size_t)D * 4;
  if (regions_clash({{work, work_bytes}}, {{x, xb}, {y, yb}, {centre, cb}})) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  float* K = (float*)(w + p.k);
  float* Z = (float*)(w + p.z);
  float* nrm = (float*)(w + p.nrm);
  hipLaunchKernelGGL(k_nn_centre, dim3(cdiv(n, 4)), dim3(256), 0, s, x, centre, Z, nrm, n, D, p.Dp);
  hipLaunchKernelGGL(k_nn_centre, dim3(cdiv(m, 4)), dim3(256), 0, s, y, centre, Z + (size_t)n * p.Dp, nrm + n, m, D, p.Dp);
  const int nbi = cdiv(p.N, NN_I), nbj = cdiv(p.Np, NN_J);
  hipLaunchKernelGGL(k_mmd_gram, dim3(nbi * nbj), dim3(256), nn_spill_bytes(k_mmd_gram, p.Dp), s, Z, nrm, p.N, p.Dp, gm,
                     n_gamma, 1.0f / (float)n_gamma, nbj, K, p.Np);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_mmd_permute_work_bytes(int n, int m, int P) {
  if (!mmd_pool_ok(n, m) || !mmd_pool_supported(n, m) || P < 1 || P > FFD_MMD_MAX_PERMUTATIONS) return 0;
  return mmd_perm_plan(n, m, P).bytes;
}

int ffd_mmd_permute(const void* gram_work, int n, int m, const uint8_t* assign, int P, double* t_out, void* work,
                    size_t work_bytes, void* stream) {
  if (!gram_work || !assign || !t_out || !work || !mmd_pool_ok(n, m) || P < 1) return FFD_ERR_INVALID;
  if (!mmd_pool_supported(n, m) || P > FFD_MMD_MAX_PERMUTATIONS) return FFD_ERR_UNSUPPORTED;
  const MmdPermPlan p = mmd_perm_plan(n, m, P);
  if (!work_ok(work, work_bytes, p.bytes) || ((uintptr_t)gram_work & 15)) return FFD_ERR_INVALID;
  const Region kmat{gram_work, (size_t)p.N * p.Np * 4}, asg{assign, (size_t)P * p.N};
  if (regions_clash({{t_out, (size_t)P * 8}, {work, work_bytes}}, {kmat, asg})) return FFD_ERR_INVALID;
  if (regions_meet(asg, kmat)) return FFD_ERR_INVALID;  // two read regions, refused all the same
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  const float* K = (const float*)gram_work;
  uint8_t* Ap = (uint8_t*)(w + p.ap);
  double* rowtot = (double*)(w + p.rowtot);
  double* part = (double*)(w + p.part);
  const size_t cells = (size_t)p.Pp * p.Np;
  hipLaunchKernelGGL(k_mmd_assign, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, assign, P, p.N, Ap, p.Pp, p.Np);
  hipLaunchKernelGGL(k_mmd_krowsum, dim3(cdiv(p.N, 4)), dim3(256), 0, s, K, p.N, p.Np, rowtot);
  hipLaunchKernelGGL(k_mmd_perm, dim3(p.nib, cdiv(p.Pp, 256)), dim3(256), 0, s, K, p.N, p.Np, Ap, p.Pp, rowtot, part);
  hipLaunchKernelGGL(k_mmd_perm_fold, dim3(cdiv(P, 256)), dim3(256), 0, s, part, p.nib, p.Pp, P, n, m, t_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"
