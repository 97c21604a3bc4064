// Entropic optimal transport between two row sets, on the device: the softmin of the squared-distance cost against a
// potential, the damped symmetric Sinkhorn loop over an epsilon schedule and the debiased Sinkhorn divergence
// (include/ffd.h ffd_sinkhorn_*; Cuturi 2013; Genevay, Peyre, Cuturi 2018; Feydy et al. 2019, Alg. 3.5).  Rows are flat
// fp32 vectors (n, D), uniform weights:
//   softmin_eps(x | y, h)_i = -eps log( (1 / nr) sum_j exp((h_j - |x_i - y_j|^2) / eps) )
//
// The pair tile is the nearest-neighbour one (ffd_pairtile.h): both sets centred on ONE caller-supplied vector, the
// exact-fp32 16x16x4 MFMA Gram form in 64 x 256 tiles, nn_d2; rows of more than NN_K_CHUNK padded columns take the
// tile's chunked sum through LDS.  No cost block goes through memory: the epilogue is an online log-sum-exp.
//   k_sk_potential  h (fp64) rounded once to fp32: what the exponent is formed from
//   k_sk_softmin    a workgroup owns 64 query rows and walks a run of SK_RUN column tiles in order.  A lane keeps, for
//                   each of its 4 rows, a running (max, sum) over ITS columns: u = h_j - d2 in fp32, the tile's maximum,
//                   one fp32 rescale of the sum where the maximum rose, then sum += exp2((u - max) c) in fp64 in
//                   (tile, b, r) order, c = log2(e) / eps rounded once; an exponent above -1/8 gives 1 + (2^t - 1) from
//                   the series (sk_exp2), so that a large eps, where every term is 1 - x, keeps x.  The four lane
//                   groups and the four waves are merged in a fixed order (sk_merge, fp64): part_m[run][i], part_s[run][i]
//   k_sk_finish     merges the runs' (max, sum) pairs in run order, out = -max - eps log(sum / nr), and the damped
//                   update out = (old + out) / 2 where `old` is given
//                   => a row's value depends on its row, the column set, the potential, the centre and eps alone: the
//                   same bits from run to run, for a query set cut in parts, whatever rows surround it
//   k_sk_radius2 + k_sk_diameter2   4 max_j |y_j - centre|^2, where a schedule starts
//   k_sk_change + k_sk_scores   max |f' - f|, |g' - g| of a pass; S = mean (f - p) + mean (g - q), fixed-order fp64 trees
// The loop is Jacobi ordered: every pass reads the previous pass's four potentials and writes four others, so for two
// equal sets the x|y and x|x passes do identical work on identical data and S is exactly 0.  No atomics anywhere.
#include <algorithm>
#include <cmath>
#include <limits>

#include "ffd_pairtile.h"

namespace ffd {

constexpr int SK_RUN = 4;  // column tiles (of 256) one workgroup walks: a constant of the source, never of the grid

// ---- softmin -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sk_potential(const double* __restrict__ h, int n, float* __restrict__ hf) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) hf[j] = (float)h[j];
}

// 2^t for t <= 0 as (value, one): the term is value + one.  Near 0 the hardware exponential's result is 1 - x rounded to
// 2^-24, which at a large eps (every exponent small) is all the information there is: eps log of the sum would carry
// eps 2^-24.  So for t > -1/8 the term is 1 + (2^t - 1) with 2^t - 1 from its series in t ln 2 (the first term left out
// is 7e-9 of it), and the ones are counted apart; elsewhere it is the hardware's 2^t.
__device__ __forceinline__ float sk_exp2(float t, int& one) {
  const float L1 = 0.693147181f, L2 = 0.240226507f, L3 = 0.0555041087f, L4 = 0.00961812911f, L5 = 0.00133335581f;
  const float e = __builtin_amdgcn_exp2f(t);
  const float p = t * __fmaf_rn(t, __fmaf_rn(t, __fmaf_rn(t, __fmaf_rn(t, L5, L4), L3), L2), L1);
  one = t > -0.125f ? 1 : 0;
  return one ? p : e;
}

// (m, s) stands for s 2^(m c): the pair for both terms.  Either maximum may be -inf with a sum of 0 (a lane none of whose
// columns lies inside the set); the weight of the pair that holds the maximum is exactly 1.
__device__ __forceinline__ void sk_merge(float& m, double& s, float m2, double s2, double c) {
  const float mx = fmaxf(m, m2);
  const double w1 = m == mx ? 1.0 : exp2(((double)m - (double)mx) * c);
  const double w2 = m2 == mx ? 1.0 : exp2(((double)m2 - (double)mx) * c);
  s = s * w1 + s2 * w2;
  m = mx;
}

// Workgroup (blockIdx.x = 64-row block, blockIdx.y = run): the (max, sum) of the run's columns for each of the rows
__global__ __launch_bounds__(256) void k_sk_softmin(const float* __restrict__ Za, const float* __restrict__ na_nrm, int na,
                                                    const float* __restrict__ Zb, const float* __restrict__ nb_nrm, int nb,
                                                    int Dp, const float* __restrict__ hf, float c, double cd, int nbj,
                                                    float* __restrict__ part_m, double* __restrict__ part_s) {
  __shared__ float red_m[4][64];
  __shared__ double red_s[4][64];
  extern __shared__ __align__(16) float sk_spill[];  // NN_SPILL_BYTES where Dp > NN_K_CHUNK, else none
  float* spill = Dp > NN_K_CHUNK ? sk_spill : nullptr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, cl = lane & 15;
  const int i0 = blockIdx.x * NN_I, run = blockIdx.y;
  const float ninf = -__builtin_inff();
  float ni[4], mx[4];
  double sum[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    ni[a] = na_nrm[min(i0 + 16 * a + cl, na - 1)];
    mx[a] = ninf;
    sum[a] = 0.0;
  }
  const int bj_hi = min(run * SK_RUN + SK_RUN, nbj);
  for (int bj = run * SK_RUN; bj < bj_hi; ++bj) {
    const int j0 = bj * NN_J + wave * 64;
    if (j0 >= nb) continue;  // (wave-uniform)
    f32x4 acc[4][4];
    nn_tile(Za, na, i0, Zb, nb, j0, Dp, q, cl, acc, spill);
    // u = h_j - d2 in place of the Gram values; -inf past the set
    float tm[4] = {ninf, ninf, ninf, ninf};
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 16 * b + 4 * q + r;
        const int jc = min(j, nb - 1);
        const float nj = nb_nrm[jc], hj = hf[jc];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const float u = j < nb ? hj - nn_d2(ni[a], nj, acc[a][b][r]) : ninf;
          acc[a][b][r] = u;
          tm[a] = fmaxf(tm[a], u);
        }
      }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float m2 = fmaxf(mx[a], tm[a]);
      if (m2 != mx[a]) {  // the maximum rose (never from -inf to -inf): the sum so far in the new unit
        int one;
        const float w = sk_exp2((mx[a] - m2) * c, one);
        sum[a] = sum[a] * (double)w + (one ? sum[a] : 0.0);
        mx[a] = m2;
      }
      int ones = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float u = acc[a][b][r];
          int one;
          const float e = sk_exp2((u - m2) * c, one);
          // (a lane with no column inside: m2 = -inf and the exponent NaN, never added)
          sum[a] += u > ninf ? (double)e : 0.0;
          ones += u > ninf ? one : 0;
        }
      sum[a] += (double)ones;
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float m = mx[a];
    double s = sum[a];
    sk_merge(m, s, __shfl_xor(m, 16, 64), __shfl_xor(s, 16, 64), cd);
    sk_merge(m, s, __shfl_xor(m, 32, 64), __shfl_xor(s, 32, 64), cd);
    if (q == 0) red_m[wave][16 * a + cl] = m, red_s[wave][16 * a + cl] = s;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int i = i0 + (int)threadIdx.x;
    if (i < na) {
      float m = red_m[0][threadIdx.x];
      double s = red_s[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < 4; ++w) sk_merge(m, s, red_m[w][threadIdx.x], red_s[w][threadIdx.x], cd);
      part_m[(size_t)run * na + i] = m;
      part_s[(size_t)run * na + i] = s;
    }
  }
}

// out[i] = -max - eps log(sum / nr) over the runs merged in run order; (old[i] + that) / 2 where old is given
__global__ __launch_bounds__(256) void k_sk_finish(const float* __restrict__ part_m, const double* __restrict__ part_s,
                                                   int nruns, int na, int nb, double eps, double cd,
                                                   const double* __restrict__ old, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= na) return;
  float m = part_m[i];
  double s = part_s[i];
  for (int r = 1; r < nruns; ++r) sk_merge(m, s, part_m[(size_t)r * na + i], part_s[(size_t)r * na + i], cd);
  const double v = -(double)m - eps * log(s / (double)nb);
  out[i] = old ? 0.5 * (old[i] + v) : v;
}

// ---- the loop's reductions -----------------------------------------------------------------------------------------
// One workgroup: out[0] = max(max_i |f1 - f0|, max_j |g1 - g0|)
__global__ __launch_bounds__(256) void k_sk_change(const double* __restrict__ f0, const double* __restrict__ f1, int n,
                                                   const double* __restrict__ g0, const double* __restrict__ g1, int m,
                                                   double* __restrict__ out) {
  __shared__ double red[256];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) v = fmax(v, fabs(f1[i] - f0[i]));
  for (int j = threadIdx.x; j < m; j += 256) v = fmax(v, fabs(g1[j] - g0[j]));
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}
// One workgroup: out[0] = mean (f - p) + mean (g - q), out[1] = mean f + mean g
__global__ __launch_bounds__(256) void k_sk_scores(const double* __restrict__ f, const double* __restrict__ p, int n,
                                                   const double* __restrict__ g, const double* __restrict__ q, int m,
                                                   double* __restrict__ out) {
  __shared__ double red[256];
  double dfp = 0.0, dgq = 0.0, sf = 0.0, sg = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) dfp += f[i] - p[i], sf += f[i];
  for (int j = threadIdx.x; j < m; j += 256) dgq += g[j] - q[j], sg += g[j];
  dfp = block_sum(dfp, red);
  dgq = block_sum(dgq, red);
  sf = block_sum(sf, red);
  sg = block_sum(sg, red);
  if (threadIdx.x == 0) {
    out[0] = dfp / (double)n + dgq / (double)m;
    out[1] = sf / (double)n + sg / (double)m;
  }
}

// ---- the schedule's diameter -----------------------------------------------------------------------------------------
// A wave per row: r2[i] = |y_i - centre|^2, the fp32 difference the tile is built from, squared and added in fp64
__global__ __launch_bounds__(256) void k_sk_radius2(const float* __restrict__ Y, const float* __restrict__ centre, int n, int D,
                                                    double* __restrict__ r2) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* y = Y + (size_t)i * D;
  double s = 0.0;
  for (int d = lane; d < D; d += 64) {
    const float z = y[d] - centre[d];
    s += (double)z * (double)z;
  }
  s = nn_wave_sum(s);
  if (lane == 0) r2[i] = s;
}
// One workgroup: out[0] = 4 max_i r2[i], the square of twice the largest radius
__global__ __launch_bounds__(256) void k_sk_diameter2(const double* __restrict__ r2, int n, double* __restrict__ out) {
  __shared__ double red[256];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) v = fmax(v, r2[i]);
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = 4.0 * red[0];
}

// ---- host: checks, workspaces --------------------------------------------------------------------------------------
// eps finite and > 0, and log2(e) / eps a normal fp32 number (the exponent's factor, rounded once)
static bool sk_eps_ok(double eps) {
  if (!std::isfinite(eps) || !(eps > 0.0)) return false;
  const float c = (float)(1.4426950408889634 / eps);
  return std::isfinite(c) && c >= std::numeric_limits<float>::min();
}

// One softmin's scratch: the potential in fp32 and the runs' (max, sum) pairs
struct SkPassPlan {
  int nruns;
  size_t hf, part_m, part_s, bytes;
};
static SkPassPlan sk_pass_plan(int na, int nb) {
  SkPassPlan p;
  p.nruns = cdiv(cdiv(nb, NN_J), SK_RUN);
  Carver c;
  p.hf = c.take((size_t)nb * 4);
  p.part_m = c.take((size_t)p.nruns * na * 4);
  p.part_s = c.take((size_t)p.nruns * na * 8);
  p.bytes = c.total;
  return p;
}
// out = softmin_eps(a | b, h), damped with `old` where given: centred rows and norms in, `scratch` of sk_pass_plan bytes
static void sk_pass(const float* Za, const float* nrm_a, int na, const float* Zb, const float* nrm_b, int nb, int Dp,
                    const double* h, double eps, const double* old, double* out, char* scratch, hipStream_t s) {
  const SkPassPlan p = sk_pass_plan(na, nb);
  float* hf = (float*)(scratch + p.hf);
  float* part_m = (float*)(scratch + p.part_m);
  double* part_s = (double*)(scratch + p.part_s);
  const double cd = 1.4426950408889634 / eps;
  hipLaunchKernelGGL(k_sk_potential, dim3(cdiv(nb, 256)), dim3(256), 0, s, h, nb, hf);
  hipLaunchKernelGGL(k_sk_softmin, dim3(cdiv(na, NN_I), p.nruns), dim3(256), nn_spill_bytes(k_sk_softmin, Dp), s, Za, nrm_a,
                     na, Zb, nrm_b, nb, Dp, hf, (float)cd, (double)(float)cd, cdiv(nb, NN_J), part_m, part_s);
  hipLaunchKernelGGL(k_sk_finish, dim3(cdiv(na, 256)), dim3(256), 0, s, part_m, part_s, p.nruns, na, nb, eps,
                     (double)(float)cd, old, out);
}

// One softmin call's workspace: the centred pair and a pass scratch
struct SkSoftminPlan {
  PairPlan pair;
  size_t pass, bytes;
};
static SkSoftminPlan sk_softmin_plan(int na, int nb, int D) {
  SkSoftminPlan p;
  Carver c;
  p.pair = nn_pair_plan(c, na, nb, D);
  p.pass = c.take(sk_pass_plan(na, nb).bytes);
  p.bytes = c.total;
  return p;
}

// The loop's workspace: both centred sets (x on the pair's reference side, y on its query side), two generations of the
// four potentials (generation 0 starts as zeros: a pass reads one generation and writes the other), one pass scratch
// sized for the largest of the four problems
struct SkLoopPlan {
  PairPlan pair;
  size_t f[2], g[2], p[2], q[2], pass, bytes;
};
static SkLoopPlan sk_loop_plan(int n, int m, int D) {
  SkLoopPlan p;
  Carver c;
  p.pair = nn_pair_plan(c, m, n, D);
  for (int k = 0; k < 2; ++k) {
    p.f[k] = c.take((size_t)n * 8);
    p.g[k] = c.take((size_t)m * 8);
    p.p[k] = c.take((size_t)n * 8);
    p.q[k] = c.take((size_t)m * 8);
  }
  const int big = std::max(n, m);
  p.pass = c.take(sk_pass_plan(big, big).bytes);
  p.bytes = c.total;
  return p;
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): entropic optimal transport ----
using namespace ffd;

extern "C" {

size_t ffd_sinkhorn_softmin_work_bytes(int nq, int nr, int D) {
  if (!nn_shape_ok(nq, nr, D) || !nn_shape_supported(nq, nr, D)) return 0;
  return sk_softmin_plan(nq, nr, D).bytes;
}

int ffd_sinkhorn_softmin(const float* query, int nq, const float* ref, int nr, int D, const float* centre, const double* h,
                         double eps, const double* old, double* out, void* work, size_t work_bytes, void* stream) {
  if (!query || !ref || !centre || !h || !out || !work || !nn_shape_ok(nq, nr, D)) return FFD_ERR_INVALID;
  if (!sk_eps_ok(eps)) return FFD_ERR_INVALID;
  if (!nn_shape_supported(nq, nr, D)) return FFD_ERR_UNSUPPORTED;
  const SkSoftminPlan p = sk_softmin_plan(nq, nr, D);
  if (!work_ok(work, work_bytes, p.bytes)) return FFD_ERR_INVALID;
  const size_t qb = (size_t)nq * D * 4, rb = (size_t)nr * D * 4, cb = (size_t)D * 4, hb = (size_t)nr * 8, ob = (size_t)nq * 8;
  if (regions_clash({{out, ob}, {work, work_bytes}}, {{query, qb}, {ref, rb}, {centre, cb}, {h, hb}, {old, ob}}))
    return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  const PairRows z = nn_centre_pair(query, nq, ref, nr, D, centre, p.pair, w, s);
  sk_pass(z.Zq, z.nrm_q, nq, z.Zr, z.nrm_r, nr, p.pair.Dp, h, eps, old, out, w + p.pass, s);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_sinkhorn_work_bytes(int n, int m, int D) {
  if (!nn_shape_ok(n, m, D) || !nn_shape_supported(n, m, D)) return 0;
  return sk_loop_plan(n, m, D).bytes;
}

int ffd_sinkhorn(const float* x, int n, const float* y, int m, int D, const float* centre, const double* eps_schedule,
                 int n_eps, const double* q_in, double* f_out, double* g_out, double* p_out, double* q_out, double* out3,
                 void* work, size_t work_bytes, void* stream) {
  if (!x || !y || !centre || !eps_schedule || !f_out || !g_out || !p_out || !q_out || !out3 || !work || !nn_shape_ok(n, m, D))
    return FFD_ERR_INVALID;
  if (n_eps < 1) return FFD_ERR_INVALID;
  for (int e = 0; e < n_eps; ++e)
    if (!sk_eps_ok(eps_schedule[e])) return FFD_ERR_INVALID;
  if (!nn_shape_supported(n, m, D)) return FFD_ERR_UNSUPPORTED;
  const SkLoopPlan pl = sk_loop_plan(n, m, D);
  if (!work_ok(work, work_bytes, pl.bytes)) return FFD_ERR_INVALID;
  const size_t xb = (size_t)n * D * 4, yb = (size_t)m * D * 4, cb = (size_t)D * 4, nb8 = (size_t)n * 8, mb8 = (size_t)m * 8;
  if (regions_clash({{f_out, nb8}, {g_out, mb8}, {p_out, nb8}, {q_out, mb8}, {out3, 24}, {work, work_bytes}},
                    {{x, xb}, {y, yb}, {centre, cb}, {q_in, mb8}}))
    return FFD_ERR_INVALID;

  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)work;
  float* Zx = (float*)(w + pl.pair.zr);
  float* Zy = (float*)(w + pl.pair.zq);
  float* nx = (float*)(w + pl.pair.nrm_r);
  float* ny = (float*)(w + pl.pair.nrm_q);
  const int Dp = pl.pair.Dp;
  double *f[2], *g[2], *p[2], *q[2];
  for (int k = 0; k < 2; ++k) {
    f[k] = (double*)(w + pl.f[k]), g[k] = (double*)(w + pl.g[k]);
    p[k] = (double*)(w + pl.p[k]), q[k] = (double*)(w + pl.q[k]);
  }
  char* scratch = w + pl.pass;
  hipLaunchKernelGGL(k_nn_centre, dim3(cdiv(n, 4)), dim3(256), 0, s, x, centre, Zx, nx, n, D, Dp);
  hipLaunchKernelGGL(k_nn_centre, dim3(cdiv(m, 4)), dim3(256), 0, s, y, centre, Zy, ny, m, D, Dp);
  // generation 0: all potentials 0 (the bytes of +0.0)
  if (hipMemsetAsync(w + pl.f[0], 0, pl.f[1] - pl.f[0], s) != hipSuccess) return FFD_ERR_HIP;
  int cur = 0;
  for (int e = 0; e < n_eps; ++e) {
    const double eps = eps_schedule[e];
    const int nxt = cur ^ 1;
    const bool damp = e > 0;  // the first pass is the softmin itself
    sk_pass(Zx, nx, n, Zy, ny, m, Dp, g[cur], eps, damp ? f[cur] : nullptr, f[nxt], scratch, s);
    sk_pass(Zy, ny, m, Zx, nx, n, Dp, f[cur], eps, damp ? g[cur] : nullptr, g[nxt], scratch, s);
    sk_pass(Zx, nx, n, Zx, nx, n, Dp, p[cur], eps, damp ? p[cur] : nullptr, p[nxt], scratch, s);
    if (!q_in) sk_pass(Zy, ny, m, Zy, ny, m, Dp, q[cur], eps, damp ? q[cur] : nullptr, q[nxt], scratch, s);
    if (e == n_eps - 1) hipLaunchKernelGGL(k_sk_change, dim3(1), dim3(256), 0, s, f[cur], f[nxt], n, g[cur], g[nxt], m, out3 + 2);
    cur = nxt;
  }
  // the extrapolation: one undamped pass at the final eps, from the last damped values
  const double eps = eps_schedule[n_eps - 1];
  sk_pass(Zx, nx, n, Zy, ny, m, Dp, g[cur], eps, nullptr, f_out, scratch, s);
  sk_pass(Zy, ny, m, Zx, nx, n, Dp, f[cur], eps, nullptr, g_out, scratch, s);
  sk_pass(Zx, nx, n, Zx, nx, n, Dp, p[cur], eps, nullptr, p_out, scratch, s);
  if (q_in) {
    if (hipMemcpyAsync(q_out, q_in, mb8, hipMemcpyDeviceToDevice, s) != hipSuccess) return FFD_ERR_HIP;
  } else {
    sk_pass(Zy, ny, m, Zy, ny, m, Dp, q[cur], eps, nullptr, q_out, scratch, s);
  }
  hipLaunchKernelGGL(k_sk_scores, dim3(1), dim3(256), 0, s, f_out, p_out, n, g_out, q_out, m, out3);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

size_t ffd_sinkhorn_diameter2_work_bytes(int n, int D) {
  if (!nn_shape_ok(n, n, D) || !nn_shape_supported(n, n, D)) return 0;
  return nn_up((size_t)n * 8, 16);
}

int ffd_sinkhorn_diameter2(const float* y, int n, int D, const float* centre, double* diameter2_out, void* work,
                           size_t work_bytes, void* stream) {
  if (!y || !centre || !diameter2_out || !work || !nn_shape_ok(n, n, D)) return FFD_ERR_INVALID;
  if (!nn_shape_supported(n, n, D)) return FFD_ERR_UNSUPPORTED;
  if (!work_ok(work, work_bytes, ffd_sinkhorn_diameter2_work_bytes(n, D))) return FFD_ERR_INVALID;
  if (regions_clash({{diameter2_out, 8}, {work, work_bytes}}, {{y, (size_t)n * D * 4}, {centre, (size_t)D * 4}}))
    return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sk_radius2, dim3(cdiv(n, 4)), dim3(256), 0, s, y, centre, n, D, (double*)work);
  hipLaunchKernelGGL(k_sk_diameter2, dim3(1), dim3(256), 0, s, (const double*)work, n, diameter2_out);
  return hipGetLastError() == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_host_sinkhorn_schedule(double diameter2, double eps_target, double scaling, int n_final, double* out, int capacity) {
  if (!std::isfinite(diameter2) || !(diameter2 > 0.0) || !std::isfinite(eps_target) || !(eps_target > 0.0)) return FFD_ERR_INVALID;
  if (!(scaling > 0.0) || !(scaling < 1.0) || n_final < 1 || capacity < 0 || (capacity > 0 && !out)) return FFD_ERR_INVALID;
  const double ratio = scaling * scaling;
  long long count = 0;
  for (double e = diameter2; e > eps_target; e *= ratio)
    if (++count > (1 << 20)) return FFD_ERR_UNSUPPORTED;
  count += n_final;
  if (count > (1 << 20)) return FFD_ERR_UNSUPPORTED;
  if (count > capacity) return (int)count;
  int k = 0;
  for (double e = diameter2; e > eps_target; e *= ratio) out[k++] = e;
  for (int i = 0; i < n_final; ++i) out[k++] = eps_target;
  return k;
}

}  // extern "C"
