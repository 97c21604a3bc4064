// Dynamic time warping between two sets of series, on the device: the k nearest references of every query under banded
// DTW, DTW of paired rows, and the six sample-quality numbers built from the searches (include/ffd.h ffd_dtw_search,
// ffd_dtw_pairs, ffd_dtw_scores).  A series is (L, C) fp32, row-major; for a Sakoe-Chiba half-width w
//   c(i, j) = sum_ch (a[i,ch] - b[j,ch])^2        fp32, ch = 0 .. C-1 in order, product and sum rounded separately
//   D(0, 0) = c(0, 0),  D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1))  over |i - j| <= w, one fp32 add
//   dtw2(a, b; w) = D(L-1, L-1)
// with every cell outside the band or the grid +inf.  A cell's value does not depend on the order the cells are visited
// in, so every tiling below gives the same bits, and the recurrence is bitwise symmetric in (a, b).
//
// A lane owns one (query, reference) pair and walks the DP rows i = 0 .. L-1 with the band of the current row in
// registers: D[k] holds column j = i - WP + k, k = 0 .. 2 WP, for the padded half-width WP of the instance
// (DTW_WIDTHS); the cells of the padded band outside the real one are +inf.  The row is updated in place in ascending k:
//   D[k] = c[k] + min3(D[k], D[k+1], D[k-1])
// where D[k] and D[k+1] still hold row i - 1 (there column j sits at k + 1 and column j - 1 at k) and D[k-1] already
// holds row i: D(i-1, j-1), D(i-1, j) and D(i, j-1).  Every loop over the band is fully unrolled, so each D[k] is one
// register.  All values are >= +0, so min3 is taken on the bit
// patterns as integers (v_min3_i32): a float min would be preceded by a quieting instruction per operand.
//   k_dtw_block   DTW_QT query rows (one per wave) x DTW_RT reference rows (one per lane) per workgroup, written into a
//                 distance block of the workspace in k_nn_tile's layout; k_nn_merge (ffd_pairtile.h) folds the block
//                 into each query row's list of the k smallest, ordered by (value, then lower index)
//   k_dtw_pairs   the same recurrence (dtw_rows) for the paired rows a[p], b[p], a wave per 64 pairs
//   k_dtw_scores  the six numbers from the search arrays, fixed-order fp64 trees in one workgroup
// Staging: the rows do not fit in LDS at L C = 65 536, so a workgroup walks time in chunks of tc <= DTW_TC rows.  For the
// DP rows [t0, t0 + tc) it stages the reference times [t0 - WP, t0 + tc + WP) transposed, element (time, channel) of
// reference r at [(time C + channel) DTW_RS + r]: the 64 lanes of a wave, which differ in r, read consecutive addresses,
// and the row stride DTW_RS = 65 keeps the transposing writes off one bank.  Times outside [0, L) are staged as +inf, so
// cells outside the grid cost +inf without a test.  The query elements are a broadcast read (k_dtw_block) or a second
// transposed tile (k_dtw_pairs).  Where even DTW_TC_MIN rows with their band do not fit in DTW_LDS_BYTES (wide bands of
// many channels), the instance reads both rows from global memory instead (STAGED = false), with the grid test explicit.
// No atomics, no cross-workgroup wait; every loop bound is a launch argument; no wave returns before a barrier.
#include <algorithm>

#include "ffd_pairtile.h"

namespace ffd {

constexpr int DTW_QT = 4;      // query rows of a workgroup of k_dtw_block: one per wave
constexpr int DTW_RT = 64;     // reference rows of a workgroup: one per lane
constexpr int DTW_RS = 65;     // floats between two (time, channel) elements of the transposed LDS tiles
constexpr int DTW_TC = 64;     // DP rows of one time chunk, at most
constexpr int DTW_TC_MIN = 8;  // below this the chunk's band costs more to stage than it saves: read from global memory
constexpr size_t DTW_LDS_BYTES = 64 * 1024;
constexpr int DTW_QBLOCK = 64, DTW_CBLOCK = 256;  // rows and columns of one unit of the distance block (k_nn_merge's)
constexpr size_t DTW_UNIT_BYTES = (size_t)DTW_QBLOCK * DTW_CBLOCK * 4;
constexpr int DTW_MAX_CBT = 32;             // column units of one distance chunk, at most (8192 columns)
constexpr size_t DTW_MAX_UNITS = 1u << 15;  // units of one distance block, at most (2 GiB)
constexpr int DTW_MAX_ROWS = 1 << 24;

__device__ __forceinline__ float dtw_min3(float a, float b, float c) {  // a, b, c >= +0 (or +inf): the integer order
  const int m = min(min(__builtin_bit_cast(int, a), __builtin_bit_cast(int, b)), __builtin_bit_cast(int, c));
  return __builtin_bit_cast(float, m);
}

// DP rows [i0, i1) of one pair.  Element (t, ch) of a is a[((t - ta0) C + ch) a_step], of b it is
// b[((t - tb0) C + ch) b_step]; STAGED: every time the band touches is inside the staged window (+inf outside the grid);
// otherwise the rows are whole (ta0 = tb0 = 0, steps 1) and times outside [0, L) are tested.  CT: C at compile time, 0 = Crt.
template <int WP, int CT, bool STAGED>
__device__ __forceinline__ void dtw_rows(float (&D)[2 * WP + 2], const float* __restrict__ a, int a_step, int ta0,
                                         const float* __restrict__ b, int b_step, int tb0, int Crt, int w, int L, int i0,
                                         int i1) {
  const int C = CT ? CT : Crt;
  const float inf = __builtin_inff();
  for (int i = i0; i < i1; ++i) {
    const float* ai = a + (size_t)(i - ta0) * C * a_step;
    const float* bi = b + ((long)(i - WP - tb0) * C) * b_step;  // band cell k = 0 is column i - WP
    float c[2 * WP + 1];
#pragma unroll
    for (int k = 0; k <= 2 * WP; ++k) c[k] = 0.f;
    for (int ch = 0; ch < C; ++ch) {
      const float av = ai[ch * a_step];
#pragma unroll
      for (int k = 0; k <= 2 * WP; ++k) {
        float bv;
        if (STAGED) {
          bv = bi[(k * C + ch) * b_step];
        } else {
          const int j = i - WP + k;
          bv = (j >= 0 && j < L) ? bi[(k * C + ch) * b_step] : inf;
        }
        const float d = av - bv;
        c[k] = __fadd_rn(c[k], __fmul_rn(d, d));
      }
    }
    float left = inf;
#pragma unroll
    for (int k = 0; k <= 2 * WP; ++k) {
      const float v = __fadd_rn(c[k], dtw_min3(D[k], D[k + 1], left));
      D[k] = (k >= WP - w && k <= WP + w) ? v : inf;  // (wave-uniform) the padded band outside the real one
      left = D[k];
    }
  }
}

template <int WP>
__device__ __forceinline__ void dtw_start(float (&D)[2 * WP + 2]) {
#pragma unroll
  for (int k = 0; k < 2 * WP + 2; ++k) D[k] = __builtin_inff();
  D[WP] = 0.f;  // D(-1, -1) = 0: row 0 then starts with D(0, 0) = c(0, 0) + 0
}

// Rows [row0, row0 + DTW_RT) of X (clamped to n - 1), elements [g0, g0 + ne) of each (element = time C + channel; those
// outside [0, LC) as +inf), transposed into tile[e DTW_RS + r].  Wave `wave` of `nwaves` takes rows wave, wave + nwaves, ...
__device__ __forceinline__ void dtw_stage(const float* __restrict__ X, int n, int row0, int LC, int g0, int ne,
                                          float* __restrict__ tile, int lane, int wave, int nwaves) {
  for (int r = wave; r < DTW_RT; r += nwaves) {
    const float* x = X + (size_t)min(row0 + r, n - 1) * LC;
    for (int e = lane; e < ne; e += 64) {
      const int g = g0 + e;
      tile[e * DTW_RS + r] = (g >= 0 && g < LC) ? x[g] : __builtin_inff();
    }
  }
}

// Workgroup blockIdx.x = bt * nct + ct: query rows [ib0 + DTW_QT bt, + DTW_QT) against reference rows
// [jc0 + DTW_RT ct, + DTW_RT).  T: (block rows, cb) floats, row = query row - ib0, column = reference row - jc0.
template <int WP, int CT, bool STAGED>
__global__ __launch_bounds__(256) void k_dtw_block(const float* __restrict__ Q, int nq, const float* __restrict__ R, int nr,
                                                   int L, int C, int w, int tc, int ib0, int jc0, int nct, int cb,
                                                   float* __restrict__ T) {
  extern __shared__ __attribute__((aligned(16))) float dtw_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bt = blockIdx.x / nct, ct = blockIdx.x - bt * nct;
  const int i = ib0 + bt * DTW_QT + wave, j0 = jc0 + ct * DTW_RT, j = j0 + lane;
  const int LC = L * C;
  const float* q = Q + (size_t)min(i, nq - 1) * LC;
  float D[2 * WP + 2];
  dtw_start<WP>(D);
  if (STAGED) {
    float* rt = dtw_lds;                              // (tc + 2 WP) C elements x DTW_RS
    float* qt = dtw_lds + (tc + 2 * WP) * C * DTW_RS;  // DTW_QT x tc C
    for (int t0 = 0; t0 < L; t0 += tc) {
      const int t1 = min(t0 + tc, L);
      __syncthreads();  // the chunk before is read
      dtw_stage(R, nr, j0, LC, (t0 - WP) * C, (t1 - t0 + 2 * WP) * C, rt, lane, wave, 4);
      for (int e = lane; e < (t1 - t0) * C; e += 64) qt[wave * tc * C + e] = q[t0 * C + e];
      __syncthreads();
      dtw_rows<WP, CT, true>(D, qt + wave * tc * C, 1, t0, rt + lane, DTW_RS, t0 - WP, C, w, L, t0, t1);
    }
  } else {
    dtw_rows<WP, CT, false>(D, q, 1, 0, R + (size_t)min(j, nr - 1) * LC, 1, 0, C, w, L, 0, L);
  }
  if (i < nq && j < nr) T[(size_t)(i - ib0) * cb + (j - jc0)] = D[WP];
}

// A wave per 64 pairs: out[p] = dtw2(a[p], b[p]; w)
template <int WP, int CT, bool STAGED>
__global__ __launch_bounds__(64) void k_dtw_pairs(const float* __restrict__ A, const float* __restrict__ B, int n, int L,
                                                  int C, int w, int tc, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float dtw_lds[];
  const int lane = threadIdx.x;
  const int p0 = blockIdx.x * DTW_RT, p = p0 + lane;
  const int LC = L * C;
  float D[2 * WP + 2];
  dtw_start<WP>(D);
  if (STAGED) {
    float* bt = dtw_lds;                              // (tc + 2 WP) C elements x DTW_RS
    float* at = dtw_lds + (tc + 2 * WP) * C * DTW_RS;  // tc C elements x DTW_RS
    for (int t0 = 0; t0 < L; t0 += tc) {
      const int t1 = min(t0 + tc, L);
      __syncthreads();
      dtw_stage(B, n, p0, LC, (t0 - WP) * C, (t1 - t0 + 2 * WP) * C, bt, lane, 0, 1);
      dtw_stage(A, n, p0, LC, t0 * C, (t1 - t0) * C, at, lane, 0, 1);
      __syncthreads();
      dtw_rows<WP, CT, true>(D, at + lane, DTW_RS, t0, bt + lane, DTW_RS, t0 - WP, C, w, L, t0, t1);
    }
  } else {
    const size_t row = (size_t)min(p, n - 1) * LC;
    dtw_rows<WP, CT, false>(D, A + row, 1, 0, B + row, 1, 0, C, w, L, 0, L);
  }
  if (p < n) out[p] = D[WP];
}

// One workgroup.  Y: the n originals, X: the m samples (include/ffd.h ffd_dtw_scores).
__global__ __launch_bounds__(256) void k_dtw_scores(const float* __restrict__ xx, const float* __restrict__ xy,
                                                    const float* __restrict__ yx, const float* __restrict__ yy,
                                                    const float* __restrict__ xy_e2, int n, int m, double* __restrict__ out) {
  __shared__ double red[256];
  double nn = 0.0, ratio = 0.0, moved = 0.0, acc_x = 0.0;
  for (int x = threadIdx.x; x < m; x += 256) {
    const double d2 = (double)xy[x], e2 = (double)xy_e2[x];
    nn += sqrt(d2);
    if (e2 > 0.0) {
      ratio += sqrt(d2 / e2);
      moved += 1.0;
    }
    acc_x += xx[x] < xy[x] ? 1.0 : 0.0;
  }
  double cov = 0.0, acc_y = 0.0;
  for (int y = threadIdx.x; y < n; y += 256) {
    cov += sqrt((double)yx[y]);
    acc_y += yy[y] < yx[y] ? 1.0 : 0.0;
  }
  nn = block_sum(nn, red);
  cov = block_sum(cov, red);
  ratio = block_sum(ratio, red);
  moved = block_sum(moved, red);
  acc_x = block_sum(acc_x, red);
  acc_y = block_sum(acc_y, red);
  if (threadIdx.x == 0) {
    out[0] = nn / (double)m;
    out[1] = cov / (double)n;
    out[2] = moved > 0.0 ? 1.0 - ratio / moved : 0.0;
    out[3] = acc_x / (double)m;
    out[4] = acc_y / (double)n;
    out[5] = 0.5 * (out[3] + out[4]);
  }
}

// ---- host: instances, workspace ----------------------------------------------------------------------------------
#define DTW_WIDTHS(X) X(0) X(4) X(8) X(16) X(32) X(64)

static int dtw_clip(int window, int L) { return std::min(window, L - 1); }
static int dtw_pad(int w) {  // the instance of a clipped window
  int wp = 0;
#define DTW_PICK(W) \
  if (wp < w) wp = W;
  DTW_WIDTHS(DTW_PICK)
#undef DTW_PICK
  return wp;
}
static size_t dtw_lds_bytes(int tc, int wp, int C, bool pairs) {
  return ((size_t)(tc + 2 * wp) * C * DTW_RS + (size_t)tc * C * (pairs ? DTW_RS : DTW_QT)) * 4;
}
// DP rows per time chunk; 0: not even DTW_TC_MIN rows fit, the rows are read from global memory
static int dtw_chunk_rows(int wp, int L, int C, bool pairs) {
  for (int tc = DTW_TC; tc >= DTW_TC_MIN; tc >>= 1)
    if (dtw_lds_bytes(std::min(tc, L), wp, C, pairs) <= DTW_LDS_BYTES) return std::min(tc, L);
  return 0;
}

template <int WP>
static void dtw_launch_block(int grid, hipStream_t s, const float* Q, int nq, const float* R, int nr, int L, int C, int w,
                             int ib0, int jc0, int nct, int cb, float* T) {
  const int tc = dtw_chunk_rows(WP, L, C, false);
  const size_t lds = tc ? dtw_lds_bytes(tc, WP, C, false) : 0;
  if (!tc)
    hipLaunchKernelGGL((k_dtw_block<WP, 0, false>), dim3(grid), dim3(256), 0, s, Q, nq, R, nr, L, C, w, tc, ib0, jc0, nct, cb, T);
  else if (C == 1)
    hipLaunchKernelGGL((k_dtw_block<WP, 1, true>), dim3(grid), dim3(256), lds, s, Q, nq, R, nr, L, C, w, tc, ib0, jc0, nct, cb, T);
  else
    hipLaunchKernelGGL((k_dtw_block<WP, 0, true>), dim3(grid), dim3(256), lds, s, Q, nq, R, nr, L, C, w, tc, ib0, jc0, nct, cb, T);
}
template <int WP>
static void dtw_launch_pairs(hipStream_t s, const float* A, const float* B, int n, int L, int C, int w, float* out) {
  const int tc = dtw_chunk_rows(WP, L, C, true), grid = cdiv(n, DTW_RT);
  const size_t lds = tc ? dtw_lds_bytes(tc, WP, C, true) : 0;
  if (!tc)
    hipLaunchKernelGGL((k_dtw_pairs<WP, 0, false>), dim3(grid), dim3(64), 0, s, A, B, n, L, C, w, tc, out);
  else if (C == 1)
    hipLaunchKernelGGL((k_dtw_pairs<WP, 1, true>), dim3(grid), dim3(64), lds, s, A, B, n, L, C, w, tc, out);
  else
    hipLaunchKernelGGL((k_dtw_pairs<WP, 0, true>), dim3(grid), dim3(64), lds, s, A, B, n, L, C, w, tc, out);
}

static size_t dtw_pow2_floor(size_t v) {
  size_t p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}
static size_t dtw_pow2_ceil(size_t v) {
  size_t p = 1;
  while (p < v) p *= 2;
  return p;
}
// column units per chunk and row units per block of the distance block that `units` 64 x 256 units allow
static void dtw_block(size_t units, int nq, int nr, int* cbt, int* qbt) {
  const int nbi = cdiv(nq, DTW_QBLOCK), nbj = cdiv(nr, DTW_CBLOCK);
  units = dtw_pow2_floor(std::max<size_t>(1, std::min(units, DTW_MAX_UNITS)));
  *cbt = (int)std::min(units, std::min<size_t>(dtw_pow2_ceil(nbj), DTW_MAX_CBT));
  *qbt = (int)std::min<size_t>(units / *cbt, nbi);
}
static bool dtw_shape_ok(int L, int C, int window) { return L >= 1 && C >= 1 && window >= 0; }
static bool dtw_shape_supported(int L, int C, int window) {
  return L <= FFD_DTW_MAX_LEN && C <= FFD_DTW_MAX_CHANNELS && (long long)L * C <= 65536 &&
         dtw_clip(window, L) <= FFD_DTW_MAX_WINDOW;
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): dynamic time warping ----
using namespace ffd;

extern "C" {

size_t ffd_dtw_work_bytes(int nq, int nr, int L, int C, int window, int k, size_t budget_bytes) {
  if (nq < 1 || nr < 1 || !dtw_shape_ok(L, C, window) || k < 1 || k > FFD_DTW_MAX_K || k > nr) return 0;
  if (nq > DTW_MAX_ROWS || nr > DTW_MAX_ROWS || !dtw_shape_supported(L, C, window)) return 0;
  int cbt, qbt;
  dtw_block(budget_bytes / DTW_UNIT_BYTES, nq, nr, &cbt, &qbt);
  return (size_t)cbt * qbt * DTW_UNIT_BYTES;
}

int ffd_dtw_search(const float* query, int nq, const float* ref, int nr, int L, int C, int window, int k, int exclude_self,
                   float* dist2_out, int32_t* index_out, void* work, size_t work_bytes, void* stream) {
  if (!query || !ref || !dist2_out || !index_out || !work || nq < 1 || nr < 1 || !dtw_shape_ok(L, C, window))
    return FFD_ERR_INVALID;
  if (k < 1 || k > FFD_DTW_MAX_K || (long long)k > (long long)nr - (exclude_self ? 1 : 0)) return FFD_ERR_INVALID;
  if (exclude_self && (query != ref || nq != nr)) return FFD_ERR_INVALID;
  if (nq > DTW_MAX_ROWS || nr > DTW_MAX_ROWS || !dtw_shape_supported(L, C, window)) return FFD_ERR_UNSUPPORTED;
  if (!work_ok(work, work_bytes, DTW_UNIT_BYTES)) return FFD_ERR_INVALID;
  const size_t qb = (size_t)nq * L * C * 4, rb = (size_t)nr * L * C * 4, db = (size_t)nq * k * 4;
  if (regions_clash({{dist2_out, db}, {index_out, db}, {work, work_bytes}}, {{query, qb}, {ref, rb}})) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int w = dtw_clip(window, L), wp = dtw_pad(w);
  float* T = (float*)work;
  int cbt, qbt;
  dtw_block(work_bytes / DTW_UNIT_BYTES, nq, nr, &cbt, &qbt);
  const int cb = cbt * DTW_CBLOCK, nbi = cdiv(nq, DTW_QBLOCK), nbj = cdiv(nr, DTW_CBLOCK);
  // the running lists are the outputs themselves: (nq, k) ascending, what k_nn_merge keeps
  for (int bi = 0; bi < nbi; bi += qbt) {
    const int ib0 = bi * DTW_QBLOCK, rows = std::min(qbt * DTW_QBLOCK, nq - ib0);
    for (int bj = 0; bj < nbj; bj += cbt) {
      const int jc0 = bj * DTW_CBLOCK, ncols = std::min(cb, nr - jc0), nct = cdiv(ncols, DTW_RT);
      const int grid = cdiv(rows, DTW_QT) * nct;
      switch (wp) {
#define DTW_CASE(W) \
  case W:           \
    dtw_launch_block<W>(grid, s, query, nq, ref, nr, L, C, w, ib0, jc0, nct, cb, T); \
    break;
        DTW_WIDTHS(DTW_CASE)
#undef DTW_CASE
      }
      hipLaunchKernelGGL(k_nn_merge, dim3(cdiv(rows, 4)), dim3(256), 0, s, T, cb, rows, ib0, jc0, ncols, exclude_self ? 1 : 0,
                         k, bj == 0 ? 1 : 0, dist2_out, index_out);
      if (hipGetLastError() != hipSuccess) return FFD_ERR_HIP;
    }
  }
  return FFD_OK;
}

int ffd_dtw_pairs(const float* a, const float* b, int n, int L, int C, int window, float* dist2_out, void* stream) {
  if (!a || !b || !dist2_out || n < 1 || !dtw_shape_ok(L, C, window)) return FFD_ERR_INVALID;
  if (n > DTW_MAX_ROWS || !dtw_shape_supported(L, C, window)) return FFD_ERR_UNSUPPORTED;
  const size_t rb = (size_t)n * L * C * 4;
  if (regions_clash({{dist2_out, (size_t)n * 4}}, {{a, rb}, {b, rb}})) return FFD_ERR_INVALID;
  const int w = dtw_clip(window, L);
  switch (dtw_pad(w)) {
#define DTW_CASE(W) \
  case W:           \
    dtw_launch_pairs<W>((hipStream_t)stream, a, b, n, L, C, w, dist2_out); \
    break;
    DTW_WIDTHS(DTW_CASE)
#undef DTW_CASE
  }
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_dtw_scores(const float* xx_d2, const float* xy_d2, const float* yx_d2, const float* yy_d2, const float* xy_e2,
                   int n_original, int m_samples, double* out6, void* stream) {
  if (!xx_d2 || !xy_d2 || !yx_d2 || !yy_d2 || !xy_e2 || !out6 || n_original < 2 || m_samples < 2) return FFD_ERR_INVALID;
  if (n_original > DTW_MAX_ROWS || m_samples > DTW_MAX_ROWS) return FFD_ERR_UNSUPPORTED;
  const size_t mb = (size_t)m_samples * 4, nb = (size_t)n_original * 4;
  if (regions_clash({{out6, 48}}, {{xx_d2, mb}, {xy_d2, mb}, {yx_d2, nb}, {yy_d2, nb}, {xy_e2, mb}})) return FFD_ERR_INVALID;
  hipLaunchKernelGGL(k_dtw_scores, dim3(1), dim3(256), 0, (hipStream_t)stream, xx_d2, xy_d2, yx_d2, yy_d2, xy_e2, n_original,
                     m_samples, out6);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"
