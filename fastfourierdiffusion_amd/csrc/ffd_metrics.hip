// Sample metrics on the device: sliced / marginal Wasserstein-2 distances between two sample sets
// (fdiff.utils.wasserstein.WassersteinDistances, wasserstein.py:95-199, with POT's ot.emd2_1d replaced by its closed
// form for uniform weights).
//
//   k_w2_project   P (K, N) = U (K, D) . X^T on the exact-fp32 16x16x4 MFMA, direction-major output
//   k_w2_columns   the marginal case: (N, D) -> (D, N) tiled transpose through LDS (x . e_i is column i exactly)
//   k_w2_sort_chunk + k_w2_merge   segmented ascending sort of K rows of N keys: 8192-key chunks by a bitonic network in
//                  LDS, then merge-path passes between runs in HBM (ping-pong between the row buffer and scratch)
//   k_w2_integral  W2^2 = integral of (a[floor(t n)] - b[floor(t m)])^2 over [0, 1] on the integer grid n m, fp64
//   k_w2_summary   mean and max of the K distances; k_col_partial + k_col_final: the column mean of a sample set
//
// Every reduction is a fixed-order tree in fp64 with no atomics: a direction's distance depends on its own row only,
// never on the launch grid or on how the directions are cut into blocks.  The ffd_w2_* / ffd_col_mean* entry points
// follow the kernels.
#include <algorithm>

#include "ffd_internal.h"

namespace ffd {

// ---- projection ------------------------------------------------------------------------------------------------
// A workgroup (4 waves) owns 64 directions x 256 rows; wave w owns rows [64 w, 64 w + 64) of it as 4 x 4 MFMA tiles.
// A = U (i = direction), B = X^T (j = row).  Both operands come straight from the row-major inputs as float4: within
// a group of 16 k values lane group q = lane >> 4 holds k = 16 g + 4 q + {0..3}, and MFMA step e pairs the e-th
// member of both -- a permutation of the k order that A and B share.  The k tail (D % 16) is loaded element-wise
// with zeros past D.  Rows / directions past the edge are clamped for the loads and never stored.
constexpr int PJ_DIRS = 64, PJ_ROWS = 256, PJ_LD = 260;  // 4 * PJ_LD % 32 == 16: the lane groups of a store hit distinct banks
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // rows of odd D are only 4-byte aligned

__device__ __forceinline__ f32x4 load_k4(const float* row, int k, int D) {
  if (k + 4 <= D) {
    f4u v = *(const f4u*)(row + k);
    return f32x4{v.x, v.y, v.z, v.w};
  }
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (k < D) v.x = row[k];
  if (k + 1 < D) v.y = row[k + 1];
  if (k + 2 < D) v.z = row[k + 2];
  return v;
}

__global__ __launch_bounds__(256) void k_w2_project(const float* __restrict__ X, const float* __restrict__ U,
                                                    float* __restrict__ P, int N, int D, int K) {
  __shared__ float tile[PJ_DIRS * PJ_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c = lane & 15;
  const int n0 = blockIdx.x * PJ_ROWS, k0 = blockIdx.y * PJ_DIRS;
  const float* xr[4];
  const float* ur[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    xr[t] = X + (size_t)min(n0 + wave * 64 + 16 * t + c, N - 1) * D;
    ur[t] = U + (size_t)min(k0 + 16 * t + c, K - 1) * D;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < D; kb += 16) {
    const int k = kb + 4 * q;
    f32x4 xa[4], ua[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      xa[t] = load_k4(xr[t], k, D);
      ua[t] = load_k4(ur[t], k, D);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = mfma16(ua[a][e], xa[b][e], acc[a][b]);
  }
  // D[i = 4 q + r][j = c]: direction 16 a + 4 q + r, row 64 wave + 16 b + c
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[(16 * a + 4 * q + r) * PJ_LD + wave * 64 + 16 * b + c] = acc[a][b][r];
  __syncthreads();
  // wave w writes directions [16 w, 16 w + 16): one 1 KiB run of a direction's row per four stores
  for (int dd = 0; dd < 16; ++dd) {
    const int dir = k0 + wave * 16 + dd;
    if (dir >= K) break;
    float* out = P + (size_t)dir * N + n0;
    const float* src = tile + (wave * 16 + dd) * PJ_LD;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = 64 * j + lane;
      if (n0 + col < N) out[col] = src[col];
    }
  }
}

// P (K, N) = U (K, D) . X (N, D)^T, direction-major
static hipError_t launch_w2_project(const float* X, const float* U, float* P, int N, int D, int K, hipStream_t s) {
  dim3 grid(cdiv(N, PJ_ROWS), cdiv(K, PJ_DIRS));
  hipLaunchKernelGGL(k_w2_project, grid, dim3(256), 0, s, X, U, P, N, D, K);
  return hipGetLastError();
}

// ---- marginal: columns f0 .. f0 + Kb of X (N, D) as rows of P (Kb, N) ------------------------------------------
__global__ __launch_bounds__(256) void k_w2_columns(const float* __restrict__ X, float* __restrict__ P, int N, int D,
                                                    int f0, int Kb) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8)
    if (n0 + r < N && c0 + tx < Kb) tile[r][tx] = X[(size_t)(n0 + r) * D + f0 + c0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (c0 + r < Kb && n0 + tx < N) P[(size_t)(c0 + r) * N + n0 + tx] = tile[tx][r];
}

// P (Kb, N) = columns [f0, f0 + Kb) of X (N, D)
hipError_t launch_w2_columns(const float* X, float* P, int N, int D, int f0, int Kb, hipStream_t s) {
  dim3 grid(cdiv(N, 32), cdiv(Kb, 32));
  hipLaunchKernelGGL(k_w2_columns, grid, dim3(256), 0, s, X, P, N, D, f0, Kb);
  return hipGetLastError();
}

// ---- segmented sort --------------------------------------------------------------------------------------------
// Keys are compared as the order-preserving unsigned image of the float (sign bit flipped for positives, all bits for
// negatives): a total order with -inf first, -0.0 before +0.0, +inf last (NaNs at the two ends).  The intermediate
// buffers hold these images; the kernel that finishes a row writes floats again.
constexpr int SORT_CHUNK = 8192, MERGE_TILE = 2048;

__device__ __forceinline__ uint32_t key_of(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// in == out is allowed: a workgroup holds its whole chunk in LDS before it writes
__global__ __launch_bounds__(1024) void k_w2_sort_chunk(const float* in, uint32_t* out, int N, int emit_float) {
  __shared__ uint32_t key[SORT_CHUNK];
  const size_t row = (size_t)blockIdx.y * N;
  const int c0 = blockIdx.x * SORT_CHUNK;
  const int cnt = min(SORT_CHUNK, N - c0);
  int S = 64;
  while (S < cnt) S <<= 1;
  for (int i = threadIdx.x; i < S; i += 1024) key[i] = i < cnt ? key_of(in[row + c0 + i]) : 0xffffffffu;
  __syncthreads();
  for (int k = 2; k <= S; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (S >> 1); t += 1024) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint32_t x = key[i], y = key[i + j];
        if ((x > y) == ((i & k) == 0)) {
          key[i] = y;
          key[i + j] = x;
        }
      }
      __syncthreads();
    }
  // the padding keys are the largest image, so the first cnt entries are the chunk's keys (an input NaN with that
  // image is indistinguishable from padding and comes back as the same bits)
  for (int i = threadIdx.x; i < cnt; i += 1024)
    out[row + c0 + i] = emit_float ? __float_as_uint(float_of(key[i])) : key[i];
}

// first d outputs of merge(A, B) take this many from A (ties: A first)
__device__ __forceinline__ int merge_split(const uint32_t* A, int na, const uint32_t* B, int nb, int d) {
  int lo = max(0, d - nb), hi = min(d, na);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One pass: runs of R sorted keys -> runs of 2 R.  A workgroup writes MERGE_TILE consecutive outputs of one row; R is a
// multiple of MERGE_TILE, so a tile lies inside one pair of runs.
__global__ __launch_bounds__(256) void k_w2_merge(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int N,
                                                  int R, int emit_float) {
  __shared__ uint32_t sin_[MERGE_TILE];
  __shared__ uint32_t sout[MERGE_TILE];
  __shared__ int cut[2];
  const size_t row = (size_t)blockIdx.y * N;
  const int o = blockIdx.x * MERGE_TILE;
  const int pb = (int)(((long long)o / (2LL * R)) * (2LL * R));
  const int a_beg = pb, a_end = (int)min((long long)pb + R, (long long)N);
  const int b_end = (int)min((long long)pb + 2LL * R, (long long)N);
  const int na = a_end - a_beg, nb = b_end - a_end;
  const uint32_t* A = in + row + a_beg;
  const uint32_t* B = in + row + a_end;
  const int d0 = o - pb, d1 = min(d0 + MERGE_TILE, na + nb);
  if (threadIdx.x == 0) cut[0] = merge_split(A, na, B, nb, d0);
  if (threadIdx.x == 64) cut[1] = merge_split(A, na, B, nb, d1);
  __syncthreads();
  const int a0 = cut[0], a1 = cut[1], b0 = d0 - a0, b1 = d1 - a1;
  const int ta = a1 - a0, tb = b1 - b0, tot = ta + tb;  // tot == d1 - d0 <= MERGE_TILE
  for (int i = threadIdx.x; i < tot; i += 256) sin_[i] = i < ta ? A[a0 + i] : B[b0 + i - ta];
  __syncthreads();
  const uint32_t* sa = sin_;
  const uint32_t* sb = sin_ + ta;
  constexpr int PER = MERGE_TILE / 256;
  const int t0 = min((int)threadIdx.x * PER, tot), t1 = min(t0 + PER, tot);
  int ia = merge_split(sa, ta, sb, tb, t0), ib = t0 - ia;
  for (int t = t0; t < t1; ++t) {
    const bool take_a = ib >= tb || (ia < ta && sa[ia] <= sb[ib]);
    sout[t] = take_a ? sa[ia++] : sb[ib++];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < tot; i += 256)
    out[row + o + i] = emit_float ? __float_as_uint(float_of(sout[i])) : sout[i];
}

// Sort the Kb rows of `rows` (Kb, N) ascending in place; `scratch` holds Kb * N more words.
hipError_t launch_w2_sort(float* rows, float* scratch, int N, int Kb, hipStream_t s) {
  int passes = 0;
  for (long long R = SORT_CHUNK; R < N; R <<= 1) ++passes;
  uint32_t* buf[2] = {(uint32_t*)rows, (uint32_t*)scratch};
  int cur = passes & 1;  // the chunk sort lands where an even number of passes remains to the row buffer
  hipLaunchKernelGGL(k_w2_sort_chunk, dim3(cdiv(N, SORT_CHUNK), Kb), dim3(1024), 0, s, rows, buf[cur], N,
                     passes == 0 ? 1 : 0);
  long long R = SORT_CHUNK;
  for (int p = 0; p < passes; ++p, R <<= 1) {
    hipLaunchKernelGGL(k_w2_merge, dim3(cdiv(N, MERGE_TILE), Kb), dim3(256), 0, s, buf[cur], buf[cur ^ 1], N, (int)R,
                       p == passes - 1 ? 1 : 0);
    cur ^= 1;
  }
  return hipGetLastError();
}

// ---- quantile integral -----------------------------------------------------------------------------------------
// One workgroup per direction.  `big` is the longer of the two sorted rows (nb >= ns): element i covers the grid
// interval [i ns, (i + 1) ns) of the n m grid, which meets at most two elements of `small` (breakpoints at multiples
// of nb).  Thread t takes i = t, t + 256, ...: the same terms in the same order whichever set is the original.
// sd_row != nullptr: the distance is divided by the population std of that row (two passes, fp64).
__global__ __launch_bounds__(256) void k_w2_integral(const float* __restrict__ big, int nb, const float* __restrict__ small,
                                                     int ns, const float* __restrict__ sd_row, int nsd,
                                                     double* __restrict__ dist) {
  __shared__ double red[256];
  const float* a = big + (size_t)blockIdx.x * nb;
  const float* b = small + (size_t)blockIdx.x * ns;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    const long long lo = (long long)i * ns, hi = lo + ns;
    const long long j = lo / nb;
    const long long brk = (j + 1) * (long long)nb;
    const double x = (double)a[i];
    const double d0 = x - (double)b[j];
    if (brk >= hi) {
      acc += (double)ns * (d0 * d0);
    } else {
      const double d1 = x - (double)b[j + 1];
      acc += (double)(brk - lo) * (d0 * d0) + (double)(hi - brk) * (d1 * d1);
    }
  }
  double w2 = block_sum(acc, red) / ((double)nb * (double)ns);
  double res = sqrt(w2);
  if (sd_row) {
    const float* r = sd_row + (size_t)blockIdx.x * nsd;
    double s1 = 0.0;
    for (int i = threadIdx.x; i < nsd; i += 256) s1 += (double)r[i];
    const double mean = block_sum(s1, red) / (double)nsd;
    double s2 = 0.0;
    for (int i = threadIdx.x; i < nsd; i += 256) {
      const double d = (double)r[i] - mean;
      s2 += d * d;
    }
    res /= sqrt(block_sum(s2, red) / (double)nsd);
  }
  if (threadIdx.x == 0) dist[blockIdx.x] = res;
}

// dist[k] = W2(pa row k (n sorted keys), pb row k (m sorted keys)) (/ population std of pa's row)
static hipError_t launch_w2_integral(const float* pa, int n, const float* pb, int m, int standardise, double* dist, int Kb,
                                     hipStream_t s) {
  const float* sd = standardise ? pa : nullptr;
  if (n >= m)
    hipLaunchKernelGGL(k_w2_integral, dim3(Kb), dim3(256), 0, s, pa, n, pb, m, sd, n, dist);
  else
    hipLaunchKernelGGL(k_w2_integral, dim3(Kb), dim3(256), 0, s, pb, m, pa, n, sd, n, dist);
  return hipGetLastError();
}

// out[0] = mean, out[1] = max of dist[0 .. K)
__global__ __launch_bounds__(256) void k_w2_summary(const double* __restrict__ dist, int K, double* __restrict__ out) {
  __shared__ double red[256];
  __shared__ double mx[256];
  double s = 0.0, m = -INFINITY;
  bool nan = false;
  for (int i = threadIdx.x; i < K; i += 256) {
    const double v = dist[i];
    s += v;
    nan |= v != v;
    m = v > m ? v : m;
  }
  mx[threadIdx.x] = nan ? (double)NAN : m;
  const double total = block_sum(s, red);
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      const double x = mx[threadIdx.x], y = mx[threadIdx.x + st];
      mx[threadIdx.x] = (x != x || y != y) ? (double)NAN : (x > y ? x : y);  // np.max propagates NaN
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = total / (double)K;
    out[1] = mx[0];
  }
}

static hipError_t launch_w2_summary(const double* dist, int K, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_w2_summary, dim3(1), dim3(256), 0, s, dist, K, out);
  return hipGetLastError();
}

// ---- column mean (the "dummy" baseline's average sample) -------------------------------------------------------
// Slabs of 1024 rows: a workgroup sums 64 columns of one slab in fp64 (4 row groups, combined in order), then one
// thread per column adds the slabs in order.  The slab size is fixed, so the grid does not change the result.
constexpr int COL_SLAB = 1024;
__global__ __launch_bounds__(256) void k_col_partial(const float* __restrict__ X, int N, int D, double* __restrict__ part) {
  __shared__ double red[4][64];
  const int cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl, g = threadIdx.x >> 6;
  const int r0 = blockIdx.y * COL_SLAB, r1 = min(r0 + COL_SLAB, N);
  double s = 0.0;
  if (c < D)
    for (int r = r0 + g; r < r1; r += 4) s += (double)X[(size_t)r * D + c];
  red[g][cl] = s;
  __syncthreads();
  if (g == 0 && c < D) part[(size_t)blockIdx.y * D + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}
__global__ __launch_bounds__(256) void k_col_final(const double* __restrict__ part, int nslab, int N, int D,
                                                   float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  double s = 0.0;
  for (int i = 0; i < nslab; ++i) s += part[(size_t)i * D + c];
  out[c] = (float)(s / (double)N);
}

static size_t col_mean_work_doubles(int N, int D) { return (size_t)cdiv(N, COL_SLAB) * D; }
static hipError_t launch_col_mean(const float* X, int N, int D, float* out, double* work, hipStream_t s) {
  const int nslab = cdiv(N, COL_SLAB);
  hipLaunchKernelGGL(k_col_partial, dim3(cdiv(D, 64), nslab), dim3(256), 0, s, X, N, D, work);
  hipLaunchKernelGGL(k_col_final, dim3(cdiv(D, 256)), dim3(256), 0, s, work, nslab, N, D, out);
  return hipGetLastError();
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): the sample metrics ----
using namespace ffd;

extern "C" {

// ---- sample metrics: sliced / marginal Wasserstein-2 (wasserstein.py:95-199) ----
// Limits: n, m <= 2^26, D <= 2^20, K <= 2^20 (FFD_ERR_UNSUPPORTED past them); a block takes at most 32768 directions.
static const int W2_MAX_N = 1 << 26, W2_MAX_D = 1 << 20, W2_MAX_K = 1 << 20, W2_MAX_BLOCK = 32768;

static size_t w2_floats_per_dir(int n, int m) {
  return m == 0 ? (size_t)n : (size_t)n + (size_t)m + (size_t)std::max(n, m);
}

static int w2_block(size_t per_dir_floats, int K, size_t work_bytes) {
  const size_t kb = work_bytes / (per_dir_floats * sizeof(float));
  return (int)std::min<size_t>(kb, (size_t)std::min(K, W2_MAX_BLOCK));
}

// rows [k0, k0 + kb) of the projected + sorted set: dirs == nullptr takes features k0 .. k0 + kb instead
static hipError_t w2_rows(const float* x, int n, int D, const float* dirs, int k0, int kb, float* dst, float* scratch,
                          hipStream_t s) {
  hipError_t e = dirs ? launch_w2_project(x, dirs + (size_t)k0 * D, dst, n, D, kb, s)
                      : launch_w2_columns(x, dst, n, D, k0, kb, s);
  if (e != hipSuccess) return e;
  return launch_w2_sort(dst, scratch, n, kb, s);
}

static int w2_check(int n, int m, int D, int K) {
  if (n < 1 || m < 1 || D < 1 || K < 1) return FFD_ERR_INVALID;
  if (n > W2_MAX_N || m > W2_MAX_N || D > W2_MAX_D || K > W2_MAX_K) return FFD_ERR_UNSUPPORTED;
  return FFD_OK;
}

size_t ffd_w2_work_bytes(int n, int m, int D, int K, size_t budget_bytes) {
  if (n < 0 || m < 0 || n + m < 1 || D < 1 || K < 1) return 0;
  const size_t per = w2_floats_per_dir(n, m) * sizeof(float);
  size_t kb = budget_bytes / per;
  kb = std::max<size_t>(1, std::min<size_t>(kb, (size_t)std::min(K, W2_MAX_BLOCK)));
  return kb * per;
}

static int w2_run(const float* orig, int n, const float* other, int m, int D, const float* dirs, int K, int standardise,
                  double* dist_out, void* work, size_t work_bytes, void* stream) {
  if (!orig || !other || !dist_out || !work) return FFD_ERR_INVALID;
  if (int rc = w2_check(n, m, D, K)) return rc;
  const int Kb = w2_block(w2_floats_per_dir(n, m), K, work_bytes);
  if (Kb < 1) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  float* pa = (float*)work;
  float* pb = pa + (size_t)Kb * n;
  float* scratch = pb + (size_t)Kb * m;
  for (int k0 = 0; k0 < K; k0 += Kb) {
    const int kb = std::min(Kb, K - k0);
    if (w2_rows(orig, n, D, dirs, k0, kb, pa, scratch, s) != hipSuccess) return FFD_ERR_HIP;
    if (w2_rows(other, m, D, dirs, k0, kb, pb, scratch, s) != hipSuccess) return FFD_ERR_HIP;
    if (launch_w2_integral(pa, n, pb, m, standardise, dist_out + k0, kb, s) != hipSuccess) return FFD_ERR_HIP;
  }
  return FFD_OK;
}

int ffd_w2_sliced(const float* orig, int n, const float* other, int m, int D, const float* dirs, int K, int standardise,
                  double* dist_out, void* work, size_t work_bytes, void* stream) {
  if (!dirs) return FFD_ERR_INVALID;
  return w2_run(orig, n, other, m, D, dirs, K, standardise, dist_out, work, work_bytes, stream);
}

int ffd_w2_marginal(const float* orig, int n, const float* other, int m, int D, int standardise, double* dist_out,
                    void* work, size_t work_bytes, void* stream) {
  return w2_run(orig, n, other, m, D, nullptr, D, standardise, dist_out, work, work_bytes, stream);
}

int ffd_w2_prepare(const float* x, int n, int D, const float* dirs, int K, float* prepared_out, void* work,
                   size_t work_bytes, void* stream) {
  if (!x || !prepared_out || !work) return FFD_ERR_INVALID;
  if (int rc = w2_check(n, 1, D, K)) return rc;
  if (!dirs && K != D) return FFD_ERR_INVALID;
  const int Kb = w2_block(w2_floats_per_dir(n, 0), K, work_bytes);
  if (Kb < 1) return FFD_ERR_INVALID;
  for (int k0 = 0; k0 < K; k0 += Kb)
    if (w2_rows(x, n, D, dirs, k0, std::min(Kb, K - k0), prepared_out + (size_t)k0 * n, (float*)work,
                (hipStream_t)stream) != hipSuccess)
      return FFD_ERR_HIP;
  return FFD_OK;
}

int ffd_w2_against_prepared(const float* prepared, int n, const float* other, int m, int D, const float* dirs, int K,
                            int standardise, double* dist_out, void* work, size_t work_bytes, void* stream) {
  if (!prepared || !other || !dist_out || !work) return FFD_ERR_INVALID;
  if (int rc = w2_check(n, m, D, K)) return rc;
  if (!dirs && K != D) return FFD_ERR_INVALID;
  const int Kb = w2_block(w2_floats_per_dir(0, m), K, work_bytes);
  if (Kb < 1) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  float* pb = (float*)work;
  float* scratch = pb + (size_t)Kb * m;
  for (int k0 = 0; k0 < K; k0 += Kb) {
    const int kb = std::min(Kb, K - k0);
    if (w2_rows(other, m, D, dirs, k0, kb, pb, scratch, s) != hipSuccess) return FFD_ERR_HIP;
    if (launch_w2_integral(prepared + (size_t)k0 * n, n, pb, m, standardise, dist_out + k0, kb, s) != hipSuccess)
      return FFD_ERR_HIP;
  }
  return FFD_OK;
}

int ffd_w2_summary(const double* dist, int K, double* mean_max_out, void* stream) {
  if (!dist || !mean_max_out || K < 1) return FFD_ERR_INVALID;
  return launch_w2_summary(dist, K, mean_max_out, (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_col_mean_work_bytes(int n, int D) {
  return n < 1 || D < 1 ? 0 : col_mean_work_doubles(n, D) * sizeof(double);
}

int ffd_col_mean(const float* x, int n, int D, float* mean_out, void* work, size_t work_bytes, void* stream) {
  if (!x || !mean_out || !work || n < 1 || D < 1 || work_bytes < ffd_col_mean_work_bytes(n, D)) return FFD_ERR_INVALID;
  if (n > W2_MAX_N / 2 || D > W2_MAX_D) return FFD_ERR_UNSUPPORTED;  // a 1024-row slab per grid row: 32768 of 65535
  return launch_col_mean(x, n, D, mean_out, (double*)work, (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

// Benchmark helper (tools/metrics_bench.py): the kernel classes of the metric one by one, HIP events around each.
int ffd_w2_bench_kernels(const float* x, int n, int D, const float* dirs, int K, float* rows, float* scratch,
                         const float* other_rows, int m, double* dist, int iters, float* ms_out, void* stream) {
  if (!x || !dirs || !rows || !scratch || !other_rows || !dist || !ms_out || iters < 1 || K > W2_MAX_BLOCK)
    return FFD_ERR_INVALID;
  if (int rc = w2_check(n, m, D, K)) return rc;
  hipStream_t s = (hipStream_t)stream;
  struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Events() {
      for (hipEvent_t ev : e)
        if (ev) (void)hipEventDestroy(ev);
    }
  } ev;
  for (hipEvent_t& e : ev.e)
    if (hipEventCreate(&e) != hipSuccess) return FFD_ERR_HIP;
  double acc[4] = {0, 0, 0, 0};
  float ms = 0.f;
  auto lap = [&](int a, int b, double& into) {
    if (hipEventElapsedTime(&ms, ev.e[a], ev.e[b]) != hipSuccess) return false;
    into += ms;
    return true;
  };
  for (int it = -1; it < iters; ++it) {  // iteration -1 warms up; the sort always meets freshly projected rows
    bool ok = hipEventRecord(ev.e[0], s) == hipSuccess && launch_w2_project(x, dirs, rows, n, D, K, s) == hipSuccess &&
              hipEventRecord(ev.e[1], s) == hipSuccess && launch_w2_sort(rows, scratch, n, K, s) == hipSuccess &&
              hipEventRecord(ev.e[2], s) == hipSuccess && hipEventSynchronize(ev.e[2]) == hipSuccess;
    double skip = 0;
    ok = ok && lap(0, 1, it < 0 ? skip : acc[0]) && lap(1, 2, it < 0 ? skip : acc[1]);
    ok = ok && hipEventRecord(ev.e[0], s) == hipSuccess &&
         launch_w2_integral(rows, n, other_rows, m, 0, dist, K, s) == hipSuccess &&
         hipEventRecord(ev.e[1], s) == hipSuccess && launch_w2_columns(x, scratch, n, D, 0, std::min(K, D), s) == hipSuccess &&
         hipEventRecord(ev.e[2], s) == hipSuccess && hipEventSynchronize(ev.e[2]) == hipSuccess;
    ok = ok && lap(0, 1, it < 0 ? skip : acc[2]) && lap(1, 2, it < 0 ? skip : acc[3]);
    if (!ok) return FFD_ERR_HIP;
  }
  for (int i = 0; i < 4; ++i) ms_out[i] = (float)(acc[i] / iters);
  return FFD_OK;
}

}  // extern "C"
