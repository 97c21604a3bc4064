// The pair tile shared by the nearest-neighbour statistics (ffd_neighbours.hip) and the kernel two-sample statistics
// (ffd_mmd.hip): a set's column mean, rows centred on a mean, one 64 x 256 tile of the centred Gram matrix on the
// exact-fp32 16x16x4 MFMA, and the one statement of d^2 from it.  Both translation units see the same bits.
//   k_nn_colpart + k_nn_colmean   a set's column mean (fp64 over fixed slabs of 1024 rows, in order)
//   k_nn_centre    z = x - mean into rows padded to a multiple of 16 columns, n_i = |z_i|^2 (a wave per row)
//   nn_tile        one 64 x 256 tile of z_q z_r^T (the operand scheme of k_ens_pairs with the reference rows as the A
//                  operand: a lane ends with 4 consecutive reference columns of one query row).  An element's sum runs
//                  over the columns in one order wherever its tile lies, so d^2(i, j) has the same bits for every tiling.
//   nn_d2          d^2 = (n_i + n_j) - 2 z_i . z_j, clamped at 0
//   k_nn_merge     a block of pair values (rows x a chunk of columns) merged into each row's list of the k smallest,
//                  ordered by nn_before: (value, then lower index); also used by ffd_dtw.hip
// Host side, for the entry points of these sources and of ffd_sinkhorn.hip and ffd_pca.hip: the shape limits, the tile
// kernels' dynamic LDS (nn_spill_bytes), the column-mean launcher, and the centred-pair layout with its launcher
// (nn_pair_plan, nn_centre_pair); the workspace helpers they stand on are ffd_workspace.h.
// The kernels are static: each translation unit that launches one carries its own copy (the library is built without
// relocatable device code).
#pragma once
#include <climits>

#include "ffd_internal.h"
#include "ffd_workspace.h"

namespace ffd {

constexpr int NN_SLAB = 1024;  // rows per column-sum slab (fixed: the grid does not change the mean)
constexpr int NN_I = 64, NN_J = 256;
constexpr int NN_MAX_ROWS = 1 << 24, NN_MAX_D = 1 << 16;

// ---- centring ----------------------------------------------------------------------------------------------------
// part[slab][d] = sum of x[i][d] over the slab's rows, fp64, 4 row groups combined in order
static __global__ __launch_bounds__(256) void k_nn_colpart(const float* __restrict__ X, int n, int D,
                                                           double* __restrict__ part) {
  __shared__ double red[4][64];
  const int cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl, g = threadIdx.x >> 6;
  const int i0 = blockIdx.y * NN_SLAB, i1 = min(i0 + NN_SLAB, n);
  double a = 0.0;
  if (c < D)
    for (int i = i0 + g; i < i1; i += 4) a += (double)X[(size_t)i * D + c];
  red[g][cl] = a;
  __syncthreads();
  if (g == 0 && c < D) part[(size_t)blockIdx.y * D + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}
// T = float: the mean the rows are centred on; T = double: the same sum and quotient, not rounded
template <typename T>
static __global__ __launch_bounds__(256) void k_nn_colmean(const double* __restrict__ part, int nslab, int n, int D,
                                                           T* __restrict__ mean) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  double a = 0.0;
  for (int i = 0; i < nslab; ++i) a += part[(size_t)i * D + c];
  mean[c] = (T)(a / (double)n);
}

__device__ __forceinline__ double nn_wave_sum(double v) {  // a fixed butterfly: every lane gets the same total
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// A wave per row: z[i][d] = x[i][d] - mean[d] (0 for D <= d < Dp), nrm[i] = |z_i|^2
static __global__ __launch_bounds__(256) void k_nn_centre(const float* __restrict__ X, const float* __restrict__ mean,
                                                          float* __restrict__ Z, float* __restrict__ nrm, int n, int D,
                                                          int Dp) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* x = X + (size_t)i * D;
  float* z = Z + (size_t)i * Dp;
  double nn = 0.0;
  for (int d = lane; d < Dp; d += 64) {
    const float zv = d < D ? x[d] - mean[d] : 0.f;
    z[d] = zv;
    nn += (double)zv * (double)zv;
  }
  nn = nn_wave_sum(nn);
  if (lane == 0) nrm[i] = (float)nn;
}

// ---- pair tiles --------------------------------------------------------------------------------------------------
// acc[a][b] of lane (q = lane >> 4, c = lane & 15), register r: z_q(i0 + 16 a + c) . z_r(j0 + 16 b + 4 q + r).  The
// reference rows are the A operand and the query rows the B operand; lane group q holds k = 16 g + 4 q + {0..3} of both,
// MFMA step e pairs the e-th of both.  Rows past the sets are clamped for the loads; the callers never use them.
// spill (nullptr: none): 64 x 256 floats of LDS, cell [slot][threadIdx.x] a lane's own.  With it the sum over k is taken
// in chunks of NN_K_CHUNK: each finished chunk's 64 partial sums are added to the lane's cells and the accumulators start
// again, so an element is ((c_1 + c_2) + ...) + the last chunk, the same wherever its tile lies, instead of one fp32 chain
// over up to 65 536 terms.  Rows of at most NN_K_CHUNK padded columns never reach a flush: the same bits as without.
constexpr int NN_K_CHUNK = 1024;
constexpr size_t NN_SPILL_BYTES = 64 * 256 * sizeof(float);
__device__ __forceinline__ void nn_tile(const float* __restrict__ Zq, int nq, int i0, const float* __restrict__ Zr, int nr,
                                        int j0, int Dp, int q, int c, f32x4 (&acc)[4][4], float* spill = nullptr) {
  const float* ar[4];
  const float* br[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    ar[t] = Zq + (size_t)min(i0 + 16 * t + c, nq - 1) * Dp + 4 * q;
    br[t] = Zr + (size_t)min(j0 + 16 * t + c, nr - 1) * Dp + 4 * q;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // (the flush sits between two inner loops, not inside one: a branch in the k loop cost a quarter of the tile's rate)
  const int chunk = spill ? NN_K_CHUNK : Dp;
  for (int k0 = 0; k0 < Dp; k0 += chunk) {
    const int k1 = min(k0 + chunk, Dp);
    for (int kb = k0; kb < k1; kb += 16) {
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
          for (int b = 0; b < 4; ++b) acc[a][b] = mfma16(bv[b][e], av[a][e], acc[a][b]);
    }
    if (spill && k1 < Dp) {  // (wave-uniform) a chunk ends and more follow
      const bool first = k0 == 0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* cell = spill + ((a * 4 + b) * 4 + r) * 256 + threadIdx.x;
            *cell = first ? acc[a][b][r] : *cell + acc[a][b][r];
            acc[a][b][r] = 0.f;
          }
    }
  }
  if (spill && Dp > NN_K_CHUNK) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][b][r] = spill[((a * 4 + b) * 4 + r) * 256 + threadIdx.x] + acc[a][b][r];
  }
}

// the one statement of the Gram form: every epilogue sees the same bits
__device__ __forceinline__ float nn_d2(float ni, float nj, float g) { return fmaxf(__fmaf_rn(-2.f, g, ni + nj), 0.f); }

// ---- the k smallest of a row ------------------------------------------------------------------------------------
// (value, index) order: a strict total order over the pairs of a row
__device__ __forceinline__ bool nn_before(float v, int j, float w, int i) { return v < w || (v == w && j < i); }

// A wave per query row of the block: lane l < k holds entry l of the row's list, ascending.  The chunk's row is read 256
// columns at a time; a column that beats the list's last entry is inserted by a shift of the lanes behind its place.
static __global__ __launch_bounds__(256) void k_nn_merge(const float* __restrict__ T, int cb, int rows, int ib0, int jc0, int ncols,
                                                         int exclude_self, int k, int first,
                                                         float* __restrict__ cand_d, int* __restrict__ cand_i) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int i = ib0 + row;
  const float* trow = T + (size_t)row * cb;
  float lv = __builtin_inff();
  int li = INT_MAX;
  if (!first && lane < k) {
    lv = cand_d[(size_t)i * k + lane];
    li = cand_i[(size_t)i * k + lane];
  }
  float wv = __shfl(lv, k - 1, 64);
  int wi = __shfl(li, k - 1, 64);
  for (int jb = 0; jb < ncols; jb += 256) {  // jb + 256 <= cb: the loads stay inside the row, the mask is `ok`
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = trow[jb + 64 * u + lane];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int jl = jb + 64 * u + lane, j = jc0 + jl;
      const bool ok = jl < ncols && !(exclude_self && j == i);
      unsigned long long m = __ballot(ok && nn_before(v[u], j, wv, wi));
      while (m) {  // (wave-uniform)
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float cv = __shfl(v[u], src, 64);
        const int cj = jc0 + jb + 64 * u + src;
        if (!nn_before(cv, cj, wv, wi)) continue;
        const int p = __popcll(__ballot(nn_before(lv, li, cv, cj)));  // the entries before the new one: a prefix, p < k
        const float uv = __shfl_up(lv, 1, 64);
        const int ui = __shfl_up(li, 1, 64);
        if (lane == p) {
          lv = cv;
          li = cj;
        } else if (lane > p) {
          lv = uv;
          li = ui;
        }
        wv = __shfl(lv, k - 1, 64);
        wi = __shfl(li, k - 1, 64);
      }
    }
  }
  if (lane < k) {
    cand_d[(size_t)i * k + lane] = lv;
    cand_i[(size_t)i * k + lane] = li;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------
// (the round-up, the workspace carver, work_ok and regions_clash: ffd_workspace.h)
static inline bool nn_shape_ok(int nq, int nr, int D) { return nq >= 1 && nr >= 1 && D >= 1; }
static inline bool nn_shape_supported(int nq, int nr, int D) {
  return nq <= NN_MAX_ROWS && nr <= NN_MAX_ROWS && D <= NN_MAX_D;
}

// Dynamic LDS of a tile kernel: the chunked sum's cells for rows of more than NN_K_CHUNK padded columns (the attribute
// lifts the kernel's limit; a failure shows as the launch's error)
template <typename K>
static size_t nn_spill_bytes(K kernel, int Dp) {
  if (Dp <= NN_K_CHUNK) return 0;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)NN_SPILL_BYTES);
  return NN_SPILL_BYTES;
}

// mean = the column mean of X (n, D), as float (what rows are centred on) or double; colpart: nn_colpart_bytes
static inline size_t nn_colpart_bytes(int n, int D) { return (size_t)cdiv(n, NN_SLAB) * D * 8; }
template <typename T>
static void nn_launch_colmean(const float* X, int n, int D, double* colpart, T* mean, hipStream_t s) {
  const int nslab = cdiv(n, NN_SLAB);
  hipLaunchKernelGGL(k_nn_colpart, dim3(cdiv(D, 64), nslab), dim3(256), 0, s, X, n, D, colpart);
  hipLaunchKernelGGL(k_nn_colmean<T>, dim3(cdiv(D, 256)), dim3(256), 0, s, (const double*)colpart, nslab, n, D, mean);
}

// The centred copies of a reference and a query set and their norms, carved in this order
struct PairPlan {
  int Dp;
  size_t zr, zq, nrm_r, nrm_q;  // byte offsets
};
static inline PairPlan nn_pair_plan(Carver& c, int nq, int nr, int D) {
  PairPlan p;
  p.Dp = (int)nn_up(D, 16);
  p.zr = c.take((size_t)nr * p.Dp * 4);
  p.zq = c.take((size_t)nq * p.Dp * 4);
  p.nrm_r = c.take((size_t)nr * 4);
  p.nrm_q = c.take((size_t)nq * 4);
  return p;
}
struct PairRows {
  const float *Zq, *nrm_q, *Zr, *nrm_r;
};
// Centres the reference rows on `centre`, and the query rows unless they are the same set: then the query side is the
// reference side's copy.
static inline PairRows nn_centre_pair(const float* query, int nq, const float* ref, int nr, int D, const float* centre,
                                      const PairPlan& p, char* work, hipStream_t s) {
  float* Zr = (float*)(work + p.zr);
  float* nrm_r = (float*)(work + p.nrm_r);
  hipLaunchKernelGGL(k_nn_centre, dim3(cdiv(nr, 4)), dim3(256), 0, s, ref, centre, Zr, nrm_r, nr, D, p.Dp);
  if (query == ref && nq == nr) return PairRows{Zr, nrm_r, Zr, nrm_r};
  float* Zq = (float*)(work + p.zq);
  float* nrm_q = (float*)(work + p.nrm_q);
  hipLaunchKernelGGL(k_nn_centre, dim3(cdiv(nq, 4)), dim3(256), 0, s, query, centre, Zq, nrm_q, nq, D, p.Dp);
  return PairRows{Zq, nrm_q, Zr, nrm_r};
}

}  // namespace ffd
