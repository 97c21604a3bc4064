// Nearest-neighbour statistics between two row sets, on the device: k-nearest-neighbour search of a query set in a
// reference set, ball counts, and the eight sample-quality numbers built from them (include/ffd.h ffd_nn_search,
// ffd_nn_ball_count, ffd_nn_scores).  Rows are flat fp32 vectors (n, D); distances are squared Euclidean.
//
// Both sets are CENTRED on the reference set's column mean before the Gram form d^2 = (n_i + n_j) - 2 z_i . z_j is taken:
// uncentred, n is the squared distance from the origin and fp32 resolves it far more coarsely than the distances between
// neighbours of a cluster away from the origin (the reason k_ens_pairs centres, ffd_ensemble.hip).
// The column mean (k_nn_colpart + k_nn_colmean), the centring (k_nn_centre), the 64 x 256 tile of z_q z_r^T on the
// exact-fp32 16x16x4 MFMA (nn_tile) and the one statement of d^2 (nn_d2) are defined in ffd_pairtile.h, which
// ffd_mmd.hip shares.  An element's sum runs over the columns in one order wherever its tile lies, so d^2(i, j) has the
// same bits for every tiling.  The merge of a distance block into each row's running list of the k smallest (k_nn_merge,
// a wave per query row, ordered by (value, then lower index): a strict total order, so the list is the same for every
// cut) is stated in ffd_pairtile.h as well; ffd_dtw.hip uses it too.  Defined here:
//   k_nn_tile      writes a block of the distance matrix (query rows x a chunk of reference columns) to the workspace
//   k_nn_refine    recomputes the k kept pairs in difference form in fp64 on the caller's rows and sorts them again
//   k_nn_ball      the same tiles with a counting epilogue: integer partial counts per (row, column chunk)
//   k_nn_count_sum folds the partial counts in chunk order
//   k_nn_scores    the eight numbers from the search / count arrays, fixed-order fp64 trees
// No atomics anywhere.
#include <algorithm>
#include <climits>

#include "ffd_pairtile.h"

namespace ffd {

constexpr int NN_MAX_CHUNKS = 64;  // (the tile, the slab and the limits: ffd_pairtile.h)
constexpr int NN_MAX_CBT = 32;              // column tiles of one distance chunk, at most (8192 columns)
constexpr size_t NN_MAX_UNITS = 1u << 15;   // 64 x 256 tiles of one distance block, at most (2 GiB)
constexpr size_t NN_UNIT_BYTES = (size_t)NN_I * NN_J * 4;

// Workgroup blockIdx.x = bt * nct + ct: query rows [ib0 + 64 bt, + 64) against reference columns [jc0 + 256 ct, + 256);
// wave w owns 64 of the columns.  T: (block rows, cb) floats, row = query row - ib0, column = reference column - jc0.
__global__ __launch_bounds__(256) void k_nn_tile(const float* __restrict__ Zq, const float* __restrict__ nq_nrm, int nq,
                                                 const float* __restrict__ Zr, const float* __restrict__ nr_nrm, int nr,
                                                 int Dp, int ib0, int jc0, int nct, int cb, float* __restrict__ T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int bt = blockIdx.x / nct, ct = blockIdx.x - bt * nct;
  const int i0 = ib0 + bt * NN_I, j0 = jc0 + ct * NN_J + wave * 64;
  if (j0 >= nr) return;  // (wave-uniform) the merge never reads these columns
  f32x4 acc[4][4];
  nn_tile(Zq, nq, i0, Zr, nr, j0, Dp, q, c, acc);
  float nj[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) nj[b][r] = nr_nrm[min(j0 + 16 * b + 4 * q + r, nr - 1)];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + 16 * a + c;
    if (i >= nq) continue;
    const float ni = nq_nrm[i];
    float* trow = T + (size_t)(i - ib0) * cb + (j0 - jc0) + 4 * q;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = nn_d2(ni, nj[b][r], acc[a][b][r]);
      *(f32x4*)(trow + 16 * b) = o;
    }
  }
}

// A wave per query row: candidate c's distance sum_d ((double)a_d - (double)b_d)^2 on the caller's rows (lane l takes
// d = l, l + 64, ..., then the butterfly), lane c keeps it; the k pairs are ranked by (value, index) and written in order.
__global__ __launch_bounds__(256) void k_nn_refine(const float* __restrict__ Q, const float* __restrict__ R, int nq, int nr,
                                                   int D, int k, const int* __restrict__ cand_i,
                                                   double* __restrict__ dist2, int32_t* __restrict__ index) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nq) return;
  const float* a = Q + (size_t)i * D;
  double myv = 0.0;
  int myi = INT_MAX;
  for (int c = 0; c < k; ++c) {
    const int idx = cand_i[(size_t)i * k + c];
    const float* b = R + (size_t)min(max(idx, 0), nr - 1) * D;  // (an index outside the set: NaN input only)
    double s = 0.0;
    for (int d = lane; d < D; d += 64) {
      const double t = (double)a[d] - (double)b[d];
      s += t * t;
    }
    s = nn_wave_sum(s);
    if (lane == c) {
      myv = s;
      myi = idx;
    }
  }
  int rank = 0;
  for (int c = 0; c < k; ++c) {
    const double ov = __shfl(myv, c, 64);
    const int oi = __shfl(myi, c, 64);
    rank += (ov < myv || (ov == myv && oi < myi)) ? 1 : 0;
  }
  if (lane < k) {
    dist2[(size_t)i * k + rank] = myv;
    index[(size_t)i * k + rank] = myi;
  }
}

// Workgroup blockIdx.x = bi * nch + ch: query rows [64 bi, + 64) against the column tiles [ch CH, ch CH + CH);
// part[ch][i] = #{ j in the chunk : d^2(i, j) <= radius2[j] }
__global__ __launch_bounds__(256) void k_nn_ball(const float* __restrict__ Zq, const float* __restrict__ nq_nrm, int nq,
                                                 const float* __restrict__ Zr, const float* __restrict__ nr_nrm, int nr,
                                                 int Dp, const float* __restrict__ radius2, int exclude_self, int nbj,
                                                 int CH, int nch, int* __restrict__ part) {
  __shared__ int red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int bi = blockIdx.x / nch, ch = blockIdx.x - bi * nch;
  const int i0 = bi * NN_I;
  float ni[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) ni[a] = nq_nrm[min(i0 + 16 * a + c, nq - 1)];
  int cnt[4] = {0, 0, 0, 0};
  const int bj_hi = min(ch * CH + CH, nbj);
  for (int bj = ch * CH; bj < bj_hi; ++bj) {
    const int j0 = bj * NN_J + wave * 64;
    if (j0 >= nr) continue;  // (wave-uniform)
    f32x4 acc[4][4];
    nn_tile(Zq, nq, i0, Zr, nr, j0, Dp, q, c, acc);
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 16 * b + 4 * q + r;
        const int jc = min(j, nr - 1);
        const float nj = nr_nrm[jc], rad = radius2[jc];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int i = i0 + 16 * a + c;
          const bool in = j < nr && !(exclude_self && i == j) && nn_d2(ni[a], nj, acc[a][b][r]) <= rad;
          cnt[a] += in ? 1 : 0;
        }
      }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int v = cnt[a];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (q == 0) red[wave][16 * a + c] = v;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int i = i0 + (int)threadIdx.x;
    if (i < nq)
      part[(size_t)ch * nq + i] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  }
}
__global__ __launch_bounds__(256) void k_nn_count_sum(const int* __restrict__ part, int nch, int nq,
                                                      int32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  int a = 0;
  for (int ch = 0; ch < nch; ++ch) a += part[(size_t)ch * nq + i];
  out[i] = a;
}

// radius2[i] = (float)dist2[i][col]: the ball-count radii from a search result
__global__ __launch_bounds__(256) void k_nn_radius(const double* __restrict__ dist2, int n, int k, int col,
                                                   float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)dist2[(size_t)i * k + col];
}

__device__ __forceinline__ double nn_block_min(double v, double* red) {  // fixed-order tree over 256 threads
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  return red[0];
}

// One workgroup.  Y: the n originals, X: the m samples (include/ffd.h ffd_nn_scores).
__global__ __launch_bounds__(256) void k_nn_scores(const double* __restrict__ self_y, const double* __restrict__ xy_d2,
                                                   const int32_t* __restrict__ xy_idx, const double* __restrict__ yx_d2,
                                                   const int32_t* __restrict__ cnt_x, const int32_t* __restrict__ cnt_y,
                                                   int n, int m, int k, double* __restrict__ out) {
  __shared__ double red[256];
  double prec = 0.0, dens = 0.0, auth = 0.0, nsum = 0.0, copies = 0.0, nmin = __builtin_inf();
  for (int x = threadIdx.x; x < m; x += 256) {
    const int cx = cnt_x[x];
    const double d2 = xy_d2[x];
    const int y = min(max(xy_idx[x], 0), n - 1);
    const double d = sqrt(d2);
    prec += cx > 0 ? 1.0 : 0.0;
    dens += (double)cx;
    auth += d2 > self_y[(size_t)y * k] ? 1.0 : 0.0;
    nsum += d;
    nmin = fmin(nmin, d);
    copies += d2 == 0.0 ? 1.0 : 0.0;
  }
  double rec = 0.0, cov = 0.0;
  for (int y = threadIdx.x; y < n; y += 256) {
    rec += cnt_y[y] > 0 ? 1.0 : 0.0;
    cov += yx_d2[y] <= self_y[(size_t)y * k + (k - 1)] ? 1.0 : 0.0;
  }
  prec = block_sum(prec, red);
  rec = block_sum(rec, red);
  dens = block_sum(dens, red);
  cov = block_sum(cov, red);
  auth = block_sum(auth, red);
  nsum = block_sum(nsum, red);
  copies = block_sum(copies, red);
  nmin = nn_block_min(nmin, red);
  if (threadIdx.x == 0) {
    out[0] = prec / (double)m;
    out[1] = rec / (double)n;
    out[2] = dens / ((double)k * (double)m);
    out[3] = cov / (double)n;
    out[4] = auth / (double)m;
    out[5] = nsum / (double)m;
    out[6] = nmin;
    out[7] = copies / (double)m;
  }
}

// ---- host: workspace, plan ---------------------------------------------------------------------------------------
static size_t nn_pow2_floor(size_t v) {
  size_t p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}
static size_t nn_pow2_ceil(size_t v) {
  size_t p = 1;
  while (p < v) p *= 2;
  return p;
}

// The fixed part of the workspace: the centred sets and their norms, the mean and its slab sums, then the running lists
// (search, k >= 1) or the partial counts (ball counts, k == 0).
struct NNPlan {
  PairPlan pair;
  int nbi, nbj;
  size_t mean, colpart, tail_a, tail_b, fixed;  // byte offsets
};
static NNPlan nn_plan(int nq, int nr, int D, int k) {
  NNPlan p;
  p.nbi = cdiv(nq, NN_I);
  p.nbj = cdiv(nr, NN_J);
  Carver c;
  p.pair = nn_pair_plan(c, nq, nr, D);
  p.mean = c.take((size_t)p.pair.Dp * 4);
  p.colpart = c.take(nn_colpart_bytes(nr, D));
  if (k > 0) {
    p.tail_a = c.take((size_t)nq * k * 4);  // cand_d
    p.tail_b = c.take((size_t)nq * k * 4);  // cand_i
  } else {
    p.tail_a = p.tail_b = c.take((size_t)std::min(p.nbj, NN_MAX_CHUNKS) * nq * 4);  // part
  }
  p.fixed = c.total;
  return p;
}
// column tiles per chunk and row tiles per block of the distance block that `units` 64 x 256 tiles allow
static void nn_block(size_t units, const NNPlan& p, int* cbt, int* qbt) {
  units = nn_pow2_floor(std::max<size_t>(1, std::min(units, NN_MAX_UNITS)));
  *cbt = (int)std::min(units, std::min<size_t>(nn_pow2_ceil(p.nbj), NN_MAX_CBT));
  *qbt = (int)std::min<size_t>(units / *cbt, p.nbi);
}
static size_t nn_search_bytes(int nq, int nr, int D, int k, size_t budget) {
  const NNPlan p = nn_plan(nq, nr, D, k);
  int cbt, qbt;
  nn_block(budget / NN_UNIT_BYTES, p, &cbt, &qbt);
  return p.fixed + (size_t)cbt * qbt * NN_UNIT_BYTES;
}
static size_t nn_ball_bytes(int nq, int nr, int D) { return nn_plan(nq, nr, D, 0).fixed; }

// the reference mean, then both sets centred on it
static hipError_t nn_centre(const float* query, int nq, const float* ref, int nr, int D, const NNPlan& p, char* work,
                            PairRows* rows, hipStream_t s) {
  float* mean = (float*)(work + p.mean);
  nn_launch_colmean(ref, nr, D, (double*)(work + p.colpart), mean, s);
  *rows = nn_centre_pair(query, nq, ref, nr, D, mean, p.pair, work, s);
  return hipGetLastError();
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): nearest-neighbour statistics ----
using namespace ffd;

extern "C" {

size_t ffd_nn_work_bytes(int nq, int nr, int D, int k, size_t budget_bytes) {
  if (!nn_shape_ok(nq, nr, D) || !nn_shape_supported(nq, nr, D) || k < 1 || k > FFD_NN_MAX_K) return 0;
  return std::max(nn_search_bytes(nq, nr, D, k, budget_bytes), nn_ball_bytes(nq, nr, D));
}

int ffd_nn_search(const float* query, int nq, const float* ref, int nr, int D, int k, int exclude_self, double* dist2_out,
                  int32_t* index_out, void* work, size_t work_bytes, void* stream) {
  if (!query || !ref || !dist2_out || !index_out || !work || !nn_shape_ok(nq, nr, D)) return FFD_ERR_INVALID;
  if (k < 1 || k > FFD_NN_MAX_K || (long long)k > (long long)nr - (exclude_self ? 1 : 0)) return FFD_ERR_INVALID;
  if (exclude_self && (query != ref || nq != nr)) return FFD_ERR_INVALID;
  if (!nn_shape_supported(nq, nr, D)) return FFD_ERR_UNSUPPORTED;
  const NNPlan p = nn_plan(nq, nr, D, k);
  if (!work_ok(work, work_bytes, p.fixed + NN_UNIT_BYTES)) return FFD_ERR_INVALID;
  const size_t qb = (size_t)nq * D * 4, rb = (size_t)nr * D * 4, db = (size_t)nq * k * 8, xb = (size_t)nq * k * 4;
  if (regions_clash({{dist2_out, db}, {index_out, xb}, {work, work_bytes}}, {{query, qb}, {ref, rb}})) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  PairRows z;
  if (nn_centre(query, nq, ref, nr, D, p, w, &z, s) != hipSuccess) return FFD_ERR_HIP;
  float* cand_d = (float*)(w + p.tail_a);
  int* cand_i = (int*)(w + p.tail_b);
  float* T = (float*)(w + p.fixed);
  int cbt, qbt;
  nn_block((work_bytes - p.fixed) / NN_UNIT_BYTES, p, &cbt, &qbt);
  const int cb = cbt * NN_J;
  for (int bi = 0; bi < p.nbi; bi += qbt) {
    const int ib0 = bi * NN_I, rows = std::min(qbt * NN_I, nq - ib0), nqt = cdiv(rows, NN_I);
    for (int bj = 0; bj < p.nbj; bj += cbt) {
      const int jc0 = bj * NN_J, nct = std::min(cbt, p.nbj - bj), ncols = std::min(cb, nr - jc0);
      hipLaunchKernelGGL(k_nn_tile, dim3(nqt * nct), dim3(256), 0, s, z.Zq, z.nrm_q, nq, z.Zr, z.nrm_r, nr,
                         p.pair.Dp, ib0, jc0, nct, cb, T);
      hipLaunchKernelGGL(k_nn_merge, dim3(cdiv(rows, 4)), dim3(256), 0, s, T, cb, rows, ib0, jc0, ncols, exclude_self ? 1 : 0,
                         k, bj == 0 ? 1 : 0, cand_d, cand_i);
      if (hipGetLastError() != hipSuccess) return FFD_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(k_nn_refine, dim3(cdiv(nq, 4)), dim3(256), 0, s, query, ref, nq, nr, D, k, cand_i, dist2_out, index_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_nn_ball_count(const float* query, int nq, const float* ref, int nr, int D, const float* radius2, int exclude_self,
                      int32_t* count_out, void* work, size_t work_bytes, void* stream) {
  if (!query || !ref || !radius2 || !count_out || !work || !nn_shape_ok(nq, nr, D)) return FFD_ERR_INVALID;
  if (exclude_self && (query != ref || nq != nr)) return FFD_ERR_INVALID;
  if (!nn_shape_supported(nq, nr, D)) return FFD_ERR_UNSUPPORTED;
  if (!work_ok(work, work_bytes, ffd_nn_work_bytes(nq, nr, D, 1, 0))) return FFD_ERR_INVALID;
  const size_t qb = (size_t)nq * D * 4, rb = (size_t)nr * D * 4, cbytes = (size_t)nq * 4, radb = (size_t)nr * 4;
  if (regions_clash({{count_out, cbytes}, {work, work_bytes}}, {{query, qb}, {ref, rb}, {radius2, radb}}))
    return FFD_ERR_INVALID;
  const NNPlan p = nn_plan(nq, nr, D, 0);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  PairRows z;
  if (nn_centre(query, nq, ref, nr, D, p, w, &z, s) != hipSuccess) return FFD_ERR_HIP;
  int* part = (int*)(w + p.tail_a);
  const int CH = cdiv(p.nbj, NN_MAX_CHUNKS), nch = cdiv(p.nbj, CH);
  hipLaunchKernelGGL(k_nn_ball, dim3(p.nbi * nch), dim3(256), 0, s, z.Zq, z.nrm_q, nq, z.Zr, z.nrm_r, nr, p.pair.Dp,
                     radius2, exclude_self ? 1 : 0, p.nbj, CH, nch, part);
  hipLaunchKernelGGL(k_nn_count_sum, dim3(cdiv(nq, 256)), dim3(256), 0, s, part, nch, nq, count_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_nn_radius(const double* dist2, int n, int k, int col, float* radius2_out, void* stream) {
  if (!dist2 || !radius2_out || n < 1 || k < 1 || k > FFD_NN_MAX_K || col < 0 || col >= k) return FFD_ERR_INVALID;
  if (regions_clash({{radius2_out, (size_t)n * 4}}, {{dist2, (size_t)n * k * 8}})) return FFD_ERR_INVALID;
  if (n > NN_MAX_ROWS) return FFD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_nn_radius, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dist2, n, k, col, radius2_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_nn_scores(const double* self_dist2, const double* xy_dist2, const int32_t* xy_index, const double* yx_dist2,
                  const int32_t* count_x, const int32_t* count_y, int n, int m, int k, double* out8, void* stream) {
  if (!self_dist2 || !xy_dist2 || !xy_index || !yx_dist2 || !count_x || !count_y || !out8) return FFD_ERR_INVALID;
  if (n < 1 || m < 1 || k < 1 || k > FFD_NN_MAX_K) return FFD_ERR_INVALID;
  if (regions_clash({{out8, 64}}, {{self_dist2, (size_t)n * k * 8},
                                   {xy_dist2, (size_t)m * 8},
                                   {xy_index, (size_t)m * 4},
                                   {yx_dist2, (size_t)n * 8},
                                   {count_x, (size_t)m * 4},
                                   {count_y, (size_t)n * 4}}))
    return FFD_ERR_INVALID;
  if (n > NN_MAX_ROWS || m > NN_MAX_ROWS) return FFD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_nn_scores, dim3(1), dim3(256), 0, (hipStream_t)stream, self_dist2, xy_dist2, xy_index, yx_dist2,
                     count_x, count_y, n, m, k, out8);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"
