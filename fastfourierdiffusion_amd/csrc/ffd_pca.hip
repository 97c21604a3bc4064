// The first two moments of a row set and what follows from them, all in float64 on the device: mean and covariance, a
// symmetric eigensolver, the symmetric square root, the Frechet distance between two fitted Gaussians
//   FD = |mu_x - mu_y|^2 + tr S_x + tr S_y - 2 tr (S_y^1/2 S_x S_y^1/2)^1/2      (Dowson & Landau 1982; Heusel et al. 2017)
// and the principal-component variances and scores (include/ffd.h ffd_cov .. ffd_pca_transform).  Rows are flat fp32
// vectors (n, D), D <= FFD_PCA_MAX_D.  Matrix products run on v_mfma_f64_16x16x4_f64 (A operand: lane holds
// A[i = lane & 15][k = lane >> 4]; B: B[k = lane >> 4][j = lane & 15]; D register r of a lane: row (lane >> 4) + 4 r, column
// lane & 15).  No atomics, no grid-wide barrier: every round is its own launch and every sum has one fixed order.
//   k_nn_colpart + k_nn_colmean<double>   the column mean (ffd_pairtile.h): a fixed-order fp64 tree over slabs of 1024 rows
//   k_pca_cov       workgroup (64 x 64 tile of the upper triangle, run of slabs): D^T D of the deviations (double)x - mean
//                   over slabs of PCA_SLAB rows, each slab from zero accumulators, the slabs of a run added in slab order
//   k_pca_cov_fold  the runs added in run order, over n - 1, entry (i, j) and (j, i) from the one value of (min, max)
//   k_pca_gemm      C = A B for strided float64 operands (A optionally fp32 rows minus a mean: the scores), k in order
//   k_eig_*         cyclic Jacobi in the round-robin order.  A round of floor(D / 2) disjoint rotations is two launches:
//                   k_eig_rot   a workgroup per pair: (c, s) from a_pp, a_qq, a_pq (Rutishauser's formulas, no rotation
//                               where a_pq == 0), stored per index as the column of J it stands for, the new diagonal
//                               a_pp - t a_pq, a_qq + t a_pq, and the rotation of rows p, q of V^T
//                   k_eig_apply a workgroup per pair: rows p, q of J^T A J from rows p, q of A and the stored rotations,
//                               into the other buffer.  Entry (i, j) is evaluated as its (min, max) orientation would be,
//                               from the same four operands, so the new matrix is symmetric bit for bit; a_pq = 0.
//                   k_eig_stat  off(A) / |A|_F by one workgroup: the 8 bytes the host reads per sweep
//                   k_eig_sort + k_eig_vectors  ascending eigenvalues (ties in index order) and their columns
//                   Every threshold is relative: a matrix times a power of two gives the same rotations bit for bit.
//   k_pca_*         small fixed-order pieces: V diag(s), mirror, (M + M^T) / 2, column dots, the five Frechet numbers
#include <algorithm>
#include <cmath>

#include "ffd_pairtile.h"

namespace ffd {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int PCA_MAX_D = FFD_PCA_MAX_D;
constexpr int PCA_MAX_ROWS = 1 << 24;
constexpr int PCA_SLAB = 256;      // rows per covariance slab: a constant of the source, never of the grid
constexpr int PCA_MAX_RUNS = 64;   // runs of consecutive slabs (a function of n alone): what bounds the workspace
constexpr int PCA_DEFAULT_SWEEPS = 30;

// ---- covariance ------------------------------------------------------------------------------------------------------
// Workgroup (blockIdx.x = 64-column block of i, blockIdx.y = 64-column block of j >= it, blockIdx.z = run): wave w rows
// i0 + 16 w .. + 16 of the tile against its 64 columns.  part[run][i][j] = sum over the run's rows of dev_i dev_j.
__global__ __launch_bounds__(256) void k_pca_cov(const float* __restrict__ X, const double* __restrict__ mean, int n, int D,
                                                 int nslab, int spr, double* __restrict__ part) {
  if (blockIdx.x > blockIdx.y) return;  // the lower triangle is the upper one's mirror (k_pca_cov_fold)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int i0 = blockIdx.x * 64 + 16 * wave, j0 = blockIdx.y * 64, run = blockIdx.z;
  const int ci = i0 + c;
  const bool oki = ci < D;
  const double mi = oki ? mean[ci] : 0.0;
  int cj[4];
  double mj[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    cj[b] = j0 + 16 * b + c;
    mj[b] = cj[b] < D ? mean[cj[b]] : 0.0;
  }
  f64x4 tot[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) tot[b] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int sl_hi = min(run * spr + spr, nslab);
  for (int sl = run * spr; sl < sl_hi; ++sl) {
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int r_lo = sl * PCA_SLAB, r_hi = min(r_lo + PCA_SLAB, n);
    for (int rb = r_lo; rb < r_hi; rb += 4) {
      const int r = rb + q;
      const bool okr = r < r_hi;
      const float* x = X + (size_t)min(r, n - 1) * D;
      const double a = okr && oki ? (double)x[ci] - mi : 0.0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double bv = okr && cj[b] < D ? (double)x[cj[b]] - mj[b] : 0.0;
        acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[b], 0, 0, 0);
      }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) tot[b] += acc[b];
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + q + 4 * r, j = cj[b];
      if (i < D && j < D) part[((size_t)run * D + i) * D + j] = tot[b][r];
    }
}
// cov[i][j] = cov[j][i] = (sum of the runs' parts at (min, max), in run order) / (n - 1)
__global__ __launch_bounds__(256) void k_pca_cov_fold(const double* __restrict__ part, int nruns, int n, int D,
                                                      double* __restrict__ cov) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= D * D) return;
  const int i = e / D, j = e - i * D, lo = min(i, j), hi = max(i, j);
  double a = 0.0;
  for (int r = 0; r < nruns; ++r) a += part[((size_t)r * D + lo) * D + hi];
  cov[e] = a / (double)(n - 1);
}

// ---- float64 products ------------------------------------------------------------------------------------------------
// C[i][j] = sum_k A(i, k) B(k, j), k ascending: A(i, k) = a[i sai + k sak] (A32: (double)fp32 a[..] - mean[k]),
// B(k, j) = b[k sbk + j sbj].  Workgroup: a 64 x 64 tile, wave w its rows 16 w .. + 16.
template <bool A32>
__global__ __launch_bounds__(256) void k_pca_gemm(const void* __restrict__ Av, long sai, long sak,
                                                  const double* __restrict__ mean, const double* __restrict__ B, long sbk,
                                                  long sbj, int M, int N, int K, double* __restrict__ C, long ldc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const long i0 = (long)blockIdx.x * 64 + 16 * wave;
  const int j0 = blockIdx.y * 64;
  if (i0 >= M) return;  // (wave-uniform)
  const long ia = i0 + c;
  const bool oki = ia < M;
  f64x4 acc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + q;
    const bool okk = k < K;
    double a = 0.0;
    if (okk && oki) {
      if (A32)
        a = (double)((const float*)Av)[ia * sai + k * sak] - mean[k];
      else
        a = ((const double*)Av)[ia * sai + k * sak];
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + 16 * b + c;
      const double bv = okk && j < N ? B[k * sbk + j * sbj] : 0.0;
      acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[b], 0, 0, 0);
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long i = i0 + q + 4 * r;
      const int j = j0 + 16 * b + c;
      if (i < M && j < N) C[i * ldc + j] = acc[b][r];
    }
}

// ---- the eigensolver -------------------------------------------------------------------------------------------------
// Round `round` of the round-robin order over np = D rounded up to even indices: pair 0 is (np - 1, round), pair k is
// ((round + k) mod (np - 1), (round - k) mod (np - 1)); p < q on return.  An index >= D is the padding of an odd D.
__device__ __host__ __forceinline__ void eig_pair(int np, int round, int k, int& p, int& q) {
  const int m = np - 1;
  int a, b;
  if (k == 0) {
    a = m, b = round;
  } else {
    a = (round + k) % m, b = (round - k + m) % m;
  }
  p = a < b ? a : b, q = a < b ? b : a;
}

// A0 = the upper triangle of a mirrored, V^T = I
__global__ __launch_bounds__(256) void k_eig_init(const double* __restrict__ a, int D, double* __restrict__ A0,
                                                  double* __restrict__ Vt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= D * D) return;
  const int i = e / D, j = e - i * D;
  A0[e] = a[(size_t)min(i, j) * D + max(i, j)];
  if (Vt) Vt[e] = i == j ? 1.0 : 0.0;
}

// One workgroup: stat[0] = off(A) / |A|_F (0 for the zero matrix), fixed-order trees
__global__ __launch_bounds__(256) void k_eig_stat(const double* __restrict__ A, int D, double* __restrict__ stat) {
  __shared__ double red[256];
  double off2 = 0.0, dg2 = 0.0;
  for (int e = threadIdx.x; e < D * D; e += 256) {
    const int i = e / D, j = e - i * D;
    const double v = A[e];
    if (i == j)
      dg2 += v * v;
    else
      off2 += v * v;
  }
  off2 = block_sum(off2, red);
  dg2 = block_sum(dg2, red);
  if (threadIdx.x == 0) {
    const double all2 = off2 + dg2;
    stat[0] = all2 > 0.0 ? sqrt(off2 / all2) : (all2 == 0.0 ? 0.0 : all2);  // (a NaN stays one)
  }
}

// Workgroup = pair: the rotation, per index the column of J it stands for ((A J)_xi = alpha_i A_xi + beta_i A_x,partner(i)),
// the new diagonal, and rows p, q of V^T
__global__ __launch_bounds__(256) void k_eig_rot(const double* __restrict__ A, int D, int np, int round,
                                                 double* __restrict__ alpha, double* __restrict__ beta,
                                                 double* __restrict__ ndiag, int* __restrict__ partner,
                                                 double* __restrict__ Vt) {
  int p, q;
  eig_pair(np, round, blockIdx.x, p, q);
  if (q >= D) {  // the padded index: p sits this round out
    if (threadIdx.x == 0 && p < D) alpha[p] = 1.0, beta[p] = 0.0, partner[p] = p, ndiag[p] = A[(size_t)p * D + p];
    return;
  }
  const double app = A[(size_t)p * D + p], aqq = A[(size_t)q * D + q], apq = A[(size_t)p * D + q];
  double c = 1.0, s = 0.0, t = 0.0;
  if (apq != 0.0) {
    const double tau = (aqq - app) / (2.0 * apq);
    t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
    c = 1.0 / sqrt(1.0 + t * t);
    s = t * c;
  }
  if (threadIdx.x == 0) {
    alpha[p] = c, beta[p] = -s, partner[p] = q, ndiag[p] = app - t * apq;
    alpha[q] = c, beta[q] = s, partner[q] = p, ndiag[q] = aqq + t * apq;
  }
  if (Vt && apq != 0.0) {
    double* vp = Vt + (size_t)p * D;
    double* vq = Vt + (size_t)q * D;
    for (int d = threadIdx.x; d < D; d += 256) {
      const double x = vp[d], y = vq[d];
      vp[d] = fma(c, x, -(s * y));
      vq[d] = fma(s, x, c * y);
    }
  }
}

// (J^T A J)_on for the outer index o and the inner index n: x00 = A_on, x01 = A_o,partner(n), x10 = A_partner(o),n,
// x11 = A_partner(o),partner(n)
__device__ __forceinline__ double eig_elem(double ao, double bo, double an, double bn, double x00, double x01, double x10,
                                           double x11) {
  const double u = fma(an, x00, bn * x01);
  const double v = fma(an, x10, bn * x11);
  return fma(ao, u, bo * v);
}

// Workgroup = pair: rows p and q of the rotated matrix into Anew (a padded pair: the one row, column rotations only)
__global__ __launch_bounds__(256) void k_eig_apply(const double* __restrict__ Aold, double* __restrict__ Anew, int D, int np,
                                                   int round, const double* __restrict__ alpha,
                                                   const double* __restrict__ beta, const double* __restrict__ ndiag,
                                                   const int* __restrict__ partner) {
  __shared__ double row[2][PCA_MAX_D];
  int p, q;
  eig_pair(np, round, blockIdx.x, p, q);
  if (p >= D) return;
  if (q >= D) q = p;
  for (int d = threadIdx.x; d < D; d += 256) {
    row[0][d] = Aold[(size_t)p * D + d];
    row[1][d] = Aold[(size_t)q * D + d];
  }
  __syncthreads();
  const int nrows = q == p ? 1 : 2;
  for (int h = 0; h < nrows; ++h) {
    const int i = h ? q : p, pi = h ? p : q;
    const double* ri = row[h];
    const double* rp = row[h ^ 1];  // (a padded pair: both rows are row p and beta_i = 0)
    const double ai = alpha[i], bi = beta[i];
    for (int j = threadIdx.x; j < D; j += 256) {
      double v;
      if (j == i) {
        v = ndiag[i];
      } else if (j == pi) {
        v = 0.0;
      } else {
        const int pj = partner[j];
        const double aj = alpha[j], bj = beta[j];
        const double x00 = ri[j], x01 = ri[pj], x10 = rp[j], x11 = rp[pj];
        v = i < j ? eig_elem(ai, bi, aj, bj, x00, x01, x10, x11) : eig_elem(aj, bj, ai, bi, x00, x10, x01, x11);
      }
      Anew[(size_t)i * D + j] = v;
    }
  }
}

// One workgroup: w[rank] = a_ii, rank = how many eigenvalues are smaller (ties: the lower index first)
__global__ __launch_bounds__(256) void k_eig_sort(const double* __restrict__ A, int D, double* __restrict__ w,
                                                  int* __restrict__ rank) {
  __shared__ double dg[PCA_MAX_D];
  for (int i = threadIdx.x; i < D; i += 256) dg[i] = A[(size_t)i * D + i];
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += 256) {
    const double v = dg[i];
    int r = 0;
    for (int j = 0; j < D; ++j) r += (dg[j] < v || (dg[j] == v && j < i)) ? 1 : 0;
    w[r] = v;
    rank[i] = r;
  }
}
// v[d][rank[i]] = Vt[i][d]
__global__ __launch_bounds__(256) void k_eig_vectors(const double* __restrict__ Vt, const int* __restrict__ rank, int D,
                                                     double* __restrict__ v) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= D * D) return;
  const int i = e / D, d = e - i * D;
  v[(size_t)d * D + rank[i]] = Vt[e];
}

// ---- small pieces ----------------------------------------------------------------------------------------------------
// T[i][k] = v[i][k] sqrt(max(w[k], 0))
__global__ __launch_bounds__(256) void k_pca_scale_cols(const double* __restrict__ v, const double* __restrict__ w, int D,
                                                        double* __restrict__ T) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= D * D) return;
  T[e] = v[e] * sqrt(fmax(w[e % D], 0.0));
}
// out[i][j] = out[j][i] = full[min][max] (half = 0), or (full[i][j] + full[j][i]) / 2 (half = 1)
__global__ __launch_bounds__(256) void k_pca_symmetrise(const double* __restrict__ full, int D, int half,
                                                        double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= D * D) return;
  const int i = e / D, j = e - i * D, lo = min(i, j), hi = max(i, j);
  const double u = full[(size_t)lo * D + hi];
  out[e] = half ? 0.5 * (u + full[(size_t)hi * D + lo]) : u;
}
// Workgroup j: out[j] = sum_d v[d][D - 1 - j] T[d][j] (T is (D, k)), a fixed-order tree
__global__ __launch_bounds__(256) void k_pca_coldot(const double* __restrict__ v, const double* __restrict__ T, int D, int k,
                                                    double* __restrict__ out) {
  __shared__ double red[256];
  const int j = blockIdx.x;
  double a = 0.0;
  for (int d = threadIdx.x; d < D; d += 256) a += v[(size_t)d * D + (D - 1 - j)] * T[(size_t)d * k + j];
  a = block_sum(a, red);
  if (threadIdx.x == 0) out[j] = a;
}
// One workgroup: out5 = {FD, |mu_x - mu_y|^2, tr S_x + tr S_y - 2 sum sqrt(max(lambda, 0)), tr S_x, tr S_y}
__global__ __launch_bounds__(256) void k_pca_frechet(const double* __restrict__ mx, const double* __restrict__ sx,
                                                     const double* __restrict__ my, const double* __restrict__ sy,
                                                     const double* __restrict__ lam, int D, double* __restrict__ out5) {
  __shared__ double red[256];
  double m2 = 0.0, tx = 0.0, ty = 0.0, rt = 0.0;
  for (int d = threadIdx.x; d < D; d += 256) {
    const double g = mx[d] - my[d];
    m2 += g * g;
    tx += sx[(size_t)d * D + d];
    ty += sy[(size_t)d * D + d];
    rt += sqrt(fmax(lam[d], 0.0));
  }
  m2 = block_sum(m2, red);
  tx = block_sum(tx, red);
  ty = block_sum(ty, red);
  rt = block_sum(rt, red);
  if (threadIdx.x == 0) {
    const double cv = (tx + ty) - 2.0 * rt;
    out5[0] = m2 + cv, out5[1] = m2, out5[2] = cv, out5[3] = tx, out5[4] = ty;
  }
}

// ---- host: checks, workspaces, the loops ---------------------------------------------------------------------------
static bool pca_d_ok(int D) { return D >= 1; }
static bool pca_d_supported(int D) { return D <= PCA_MAX_D; }
static size_t pca_mat(int D) { return nn_up((size_t)D * D * 8, 16); }
static size_t pca_vec(int D) { return nn_up((size_t)D * 8, 16); }

struct CovPlan {
  int nslab, spr, nruns;
  size_t mean_part, part, bytes;
};
static CovPlan cov_plan(int n, int D) {
  CovPlan p;
  p.nslab = cdiv(n, PCA_SLAB);
  p.spr = cdiv(p.nslab, PCA_MAX_RUNS);
  p.nruns = cdiv(p.nslab, p.spr);
  Carver c;
  p.mean_part = c.take(nn_colpart_bytes(n, D));
  // (PCA_MAX_RUNS parts for every n, so that the need never falls as n grows)
  p.part = c.take((size_t)PCA_MAX_RUNS * pca_mat(D));
  p.bytes = c.total;
  return p;
}

static void pca_gemm(const double* A, long sai, long sak, const double* B, long sbk, long sbj, int M, int N, int K, double* C,
                     long ldc, hipStream_t s) {
  hipLaunchKernelGGL(k_pca_gemm<false>, dim3(cdiv(M, 64), cdiv(N, 64)), dim3(256), 0, s, (const void*)A, sai, sak,
                     (const double*)nullptr, B, sbk, sbj, M, N, K, C, ldc);
}

struct EigPlan {
  size_t a0, a1, vt, alpha, beta, ndiag, partner, rank, stat, bytes;
};
static EigPlan eig_plan(int D) {
  EigPlan p;
  Carver c;
  p.a0 = c.take(pca_mat(D));
  p.a1 = c.take(pca_mat(D));
  p.vt = c.take(pca_mat(D));
  p.alpha = c.take(pca_vec(D));
  p.beta = c.take(pca_vec(D));
  p.ndiag = c.take(pca_vec(D));
  p.partner = c.take(pca_vec(D));
  p.rank = c.take(pca_vec(D));
  p.stat = c.take(16);
  p.bytes = c.total;
  return p;
}
// The sweeps on `a` (its upper triangle), w and optionally v out; info = {sweeps done, off / |A|_F at the end, 1 if that
// is <= 2^-53}.  Reads 8 bytes back per sweep: synchronises the stream.
static int eig_run(const double* a, int D, int max_sweeps, double* w_out, double* v_out, char* w, hipStream_t s,
                   double* info) {
  const EigPlan p = eig_plan(D);
  double* A[2] = {(double*)(w + p.a0), (double*)(w + p.a1)};
  double* Vt = v_out ? (double*)(w + p.vt) : nullptr;
  double* alpha = (double*)(w + p.alpha);
  double* beta = (double*)(w + p.beta);
  double* ndiag = (double*)(w + p.ndiag);
  int* partner = (int*)(w + p.partner);
  int* rank = (int*)(w + p.rank);
  double* stat = (double*)(w + p.stat);
  const int grid = cdiv(D * D, 256), np = D + (D & 1), rounds = np - 1;
  hipLaunchKernelGGL(k_eig_init, dim3(grid), dim3(256), 0, s, a, D, A[0], Vt);
  int cur = 0, sweeps = 0;
  double ratio = 0.0;
  bool done = false;
  for (;;) {
    hipLaunchKernelGGL(k_eig_stat, dim3(1), dim3(256), 0, s, (const double*)A[cur], D, stat);
    if (hipMemcpyAsync(&ratio, stat, 8, hipMemcpyDeviceToHost, s) != hipSuccess) return FFD_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return FFD_ERR_HIP;
    done = ratio <= 0x1p-53;
    if (done || sweeps == max_sweeps) break;
    for (int r = 0; r < rounds; ++r) {
      hipLaunchKernelGGL(k_eig_rot, dim3(np / 2), dim3(256), 0, s, (const double*)A[cur], D, np, r, alpha, beta, ndiag,
                         partner, Vt);
      hipLaunchKernelGGL(k_eig_apply, dim3(np / 2), dim3(256), 0, s, (const double*)A[cur], A[cur ^ 1], D, np, r,
                         (const double*)alpha, (const double*)beta, (const double*)ndiag, (const int*)partner);
      cur ^= 1;
    }
    ++sweeps;
  }
  hipLaunchKernelGGL(k_eig_sort, dim3(1), dim3(256), 0, s, (const double*)A[cur], D, w_out, rank);
  if (v_out) hipLaunchKernelGGL(k_eig_vectors, dim3(grid), dim3(256), 0, s, (const double*)Vt, (const int*)rank, D, v_out);
  info[0] = (double)sweeps, info[1] = ratio, info[2] = done ? 1.0 : 0.0;
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

// root = V diag(sqrt(max(w, 0))) V^T through T = V diag(..) (scratch: one matrix for T, one for the full product)
static void root_run(const double* w, const double* v, int D, double* root, double* T, double* full, hipStream_t s) {
  const int grid = cdiv(D * D, 256);
  hipLaunchKernelGGL(k_pca_scale_cols, dim3(grid), dim3(256), 0, s, v, w, D, T);
  pca_gemm(T, D, 1, v, 1, D, D, D, D, full, D, s);  // B(k, j) = v[j][k]
  hipLaunchKernelGGL(k_pca_symmetrise, dim3(grid), dim3(256), 0, s, (const double*)full, D, 0, root);
}

struct FrechetPlan {
  size_t eig, w, v, root, t1, t2, bytes;
};
static FrechetPlan frechet_plan(int D) {
  FrechetPlan p;
  Carver c;
  p.eig = c.take(eig_plan(D).bytes);
  p.w = c.take(pca_vec(D));
  p.v = c.take(pca_mat(D));
  p.root = c.take(pca_mat(D));
  p.t1 = c.take(pca_mat(D));
  p.t2 = c.take(pca_mat(D));
  p.bytes = c.total;
  return p;
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): moments, eigenvalues, the Frechet distance, principal components ----
using namespace ffd;

extern "C" {

size_t ffd_cov_work_bytes(int n, int D) {
  if (n < 2 || !pca_d_ok(D) || n > PCA_MAX_ROWS || !pca_d_supported(D)) return 0;
  return cov_plan(n, D).bytes;
}

int ffd_cov(const float* x, int n, int D, double* mean_out, double* cov_out, void* work, size_t work_bytes, void* stream) {
  if (!x || !mean_out || !cov_out || !work || n < 2 || !pca_d_ok(D)) return FFD_ERR_INVALID;
  if (n > PCA_MAX_ROWS || !pca_d_supported(D)) return FFD_ERR_UNSUPPORTED;
  const CovPlan p = cov_plan(n, D);
  if (!work_ok(work, work_bytes, p.bytes)) return FFD_ERR_INVALID;
  const size_t vb = (size_t)D * 8, mb = (size_t)D * D * 8;
  if (regions_clash({{mean_out, vb}, {cov_out, mb}, {work, work_bytes}}, {{x, (size_t)n * D * 4}})) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  double* part = (double*)(w + p.part);
  nn_launch_colmean(x, n, D, (double*)(w + p.mean_part), mean_out, s);
  const int nt = cdiv(D, 64);
  hipLaunchKernelGGL(k_pca_cov, dim3(nt, nt, p.nruns), dim3(256), 0, s, x, (const double*)mean_out, n, D, p.nslab, p.spr,
                     part);
  hipLaunchKernelGGL(k_pca_cov_fold, dim3(cdiv(D * D, 256)), dim3(256), 0, s, (const double*)part, p.nruns, n, D, cov_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_sym_eig_work_bytes(int D) {
  if (!pca_d_ok(D) || !pca_d_supported(D)) return 0;
  return eig_plan(D).bytes;
}

int ffd_sym_eig(const double* a, int D, int max_sweeps, double* w_out, double* v_out, double* info3_host, void* work,
                size_t work_bytes, void* stream) {
  if (!a || !w_out || !info3_host || !work || !pca_d_ok(D) || max_sweeps < 0) return FFD_ERR_INVALID;
  if (!pca_d_supported(D)) return FFD_ERR_UNSUPPORTED;
  if (!work_ok(work, work_bytes, eig_plan(D).bytes)) return FFD_ERR_INVALID;
  const size_t vb = (size_t)D * 8, mb = (size_t)D * D * 8;
  if (regions_clash({{w_out, vb}, {v_out, mb}, {work, work_bytes}}, {{a, mb}})) return FFD_ERR_INVALID;
  return eig_run(a, D, max_sweeps ? max_sweeps : PCA_DEFAULT_SWEEPS, w_out, v_out, (char*)work, (hipStream_t)stream,
                 info3_host);
}

size_t ffd_sym_root_work_bytes(int D) {
  if (!pca_d_ok(D) || !pca_d_supported(D)) return 0;
  return 2 * pca_mat(D);
}

int ffd_sym_root(const double* w, const double* v, int D, double* root_out, void* work, size_t work_bytes, void* stream) {
  if (!w || !v || !root_out || !work || !pca_d_ok(D)) return FFD_ERR_INVALID;
  if (!pca_d_supported(D)) return FFD_ERR_UNSUPPORTED;
  if (!work_ok(work, work_bytes, 2 * pca_mat(D))) return FFD_ERR_INVALID;
  const size_t vb = (size_t)D * 8, mb = (size_t)D * D * 8;
  if (regions_clash({{root_out, mb}, {work, work_bytes}}, {{w, vb}, {v, mb}})) return FFD_ERR_INVALID;
  char* wk = (char*)work;
  root_run(w, v, D, root_out, (double*)wk, (double*)(wk + pca_mat(D)), (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_frechet_work_bytes(int D) {
  if (!pca_d_ok(D) || !pca_d_supported(D)) return 0;
  return frechet_plan(D).bytes;
}

int ffd_frechet(const double* mean_x, const double* cov_x, const double* mean_y, const double* cov_y, const double* root_y,
                int D, int max_sweeps, double* out5, double* info3_host, void* work, size_t work_bytes, void* stream) {
  if (!mean_x || !cov_x || !mean_y || !cov_y || !out5 || !info3_host || !work || !pca_d_ok(D) || max_sweeps < 0)
    return FFD_ERR_INVALID;
  if (!pca_d_supported(D)) return FFD_ERR_UNSUPPORTED;
  const FrechetPlan p = frechet_plan(D);
  if (!work_ok(work, work_bytes, p.bytes)) return FFD_ERR_INVALID;
  const size_t vb = (size_t)D * 8, mb = (size_t)D * D * 8;
  if (regions_clash({{out5, 40}, {work, work_bytes}}, {{mean_x, vb}, {cov_x, mb}, {mean_y, vb}, {cov_y, mb}, {root_y, mb}}))
    return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  char* wk = (char*)work;
  double* lam = (double*)(wk + p.w);
  double* V = (double*)(wk + p.v);
  double* root = (double*)(wk + p.root);
  double* t1 = (double*)(wk + p.t1);
  double* t2 = (double*)(wk + p.t2);
  const int cap = max_sweeps ? max_sweeps : PCA_DEFAULT_SWEEPS;
  double info[3] = {0.0, 0.0, 1.0}, worst[3] = {0.0, 0.0, 1.0};
  const double* R = root_y;
  if (!R) {
    const int rc = eig_run(cov_y, D, cap, lam, V, wk + p.eig, s, info);
    if (rc != FFD_OK) return rc;
    worst[0] = info[0], worst[1] = info[1], worst[2] = info[2];
    root_run(lam, V, D, root, t1, t2, s);
    R = root;
  }
  // M = R S_x R from two products, then (M + M^T) / 2
  pca_gemm(cov_x, D, 1, R, D, 1, D, D, D, t1, D, s);
  pca_gemm(R, D, 1, t1, D, 1, D, D, D, t2, D, s);
  hipLaunchKernelGGL(k_pca_symmetrise, dim3(cdiv(D * D, 256)), dim3(256), 0, s, (const double*)t2, D, 1, t1);
  const int rc = eig_run(t1, D, cap, lam, nullptr, wk + p.eig, s, info);
  if (rc != FFD_OK) return rc;
  worst[0] = std::max(worst[0], info[0]);
  worst[1] = info[1] <= worst[1] ? worst[1] : info[1];  // (a NaN wins)
  worst[2] = std::min(worst[2], info[2]);
  hipLaunchKernelGGL(k_pca_frechet, dim3(1), dim3(256), 0, s, mean_x, cov_x, mean_y, cov_y, (const double*)lam, D, out5);
  if (hipGetLastError() != hipSuccess) return FFD_ERR_HIP;
  info3_host[0] = worst[0], info3_host[1] = worst[1], info3_host[2] = worst[2];
  return FFD_OK;
}

size_t ffd_pca_variances_work_bytes(int D, int k) {
  if (!pca_d_ok(D) || !pca_d_supported(D) || k < 1 || k > D) return 0;
  return nn_up((size_t)D * k * 8, 16);
}

int ffd_pca_variances(const double* cov, const double* v, int D, int k, double* out, void* work, size_t work_bytes,
                      void* stream) {
  if (!cov || !v || !out || !work || !pca_d_ok(D) || k < 1) return FFD_ERR_INVALID;
  if (!pca_d_supported(D)) return FFD_ERR_UNSUPPORTED;
  if (k > D) return FFD_ERR_INVALID;
  if (!work_ok(work, work_bytes, nn_up((size_t)D * k * 8, 16))) return FFD_ERR_INVALID;
  const size_t mb = (size_t)D * D * 8;
  if (regions_clash({{out, (size_t)k * 8}, {work, work_bytes}}, {{cov, mb}, {v, mb}})) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  double* T = (double*)work;
  pca_gemm(cov, D, 1, v + (D - 1), D, -1, D, k, D, T, k, s);  // B(d, j) = v[d][D - 1 - j]
  hipLaunchKernelGGL(k_pca_coldot, dim3(k), dim3(256), 0, s, v, (const double*)T, D, k, out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_pca_transform(const float* x, int n, int D, const double* mean, const double* v, int k, double* scores_out,
                      void* stream) {
  if (!x || !mean || !v || !scores_out || n < 1 || !pca_d_ok(D) || k < 1) return FFD_ERR_INVALID;
  if (n > PCA_MAX_ROWS || !pca_d_supported(D)) return FFD_ERR_UNSUPPORTED;
  if (k > D) return FFD_ERR_INVALID;
  if (regions_clash({{scores_out, (size_t)n * k * 8}}, {{x, (size_t)n * D * 4}, {mean, (size_t)D * 8}, {v, (size_t)D * D * 8}}))
    return FFD_ERR_INVALID;
  hipLaunchKernelGGL(k_pca_gemm<true>, dim3(cdiv(n, 64), cdiv(k, 64)), dim3(256), 0, (hipStream_t)stream, (const void*)x,
                     (long)D, 1L, mean, v + (D - 1), (long)D, -1L, n, k, D, scores_out, (long)k);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"
