// Class-conditional score models and classifier-free guidance (include/ffd.h ffd_class_temb, ffd_cfg_combine,
// ffd_class_drop, ffd_class_table_grad): the small operators around the unchanged network kernels.
//   k_class_temb        the per-sample embedding rows temb + table[label] of one evaluation (conditional block, and with
//                       `stack` the null block behind it); the same launch copies x into both halves of the stacked batch
//   k_cfg_combine       c <- u + g (c - u) in place, float4 where c and u share their 16-byte phase
//   k_class_drop        the label dropout, keyed by the global row like the loss's time draws
//   k_class_table_grad  the table's gradient: a thread per (class, column), the batch walked in order in fp64
// All of them are memory-bound and tiny next to a forward (the table build is B d floats, the combine B L d at most).
// The context state that uses them is in ffd_api.hip, the training forward / backward in ffd_train.hip.
#include <cmath>

#include "ffd_internal.h"

namespace ffd {

__device__ __forceinline__ int class_row(const int32_t* labels, int r, int n_classes) {
  const int y = labels ? labels[r] : n_classes;
  return y < 0 || y > n_classes ? n_classes : y;  // -1, n_classes (and anything outside): the null row
}

__global__ __launch_bounds__(256) void k_class_temb(const float* temb, int temb_stride, const float* __restrict__ table,
                                                    int n_classes, const int32_t* __restrict__ labels, int B, int d, int rows,
                                                    float* out, const float* __restrict__ x, float* __restrict__ xs,
                                                    size_t nx) {
  const size_t ne = (size_t)rows * d, total = ne + (xs ? nx : 0);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    if (i < ne) {
      const int r = (int)(i / d), j = (int)(i - (size_t)r * d);
      const int b = r < B ? r : r - B;
      const int y = r < B ? class_row(labels, b, n_classes) : n_classes;
      out[i] = __fadd_rn(temb[(size_t)b * temb_stride + j], table[(size_t)y * d + j]);
    } else {
      const size_t k = i - ne;
      const float v = x[k];
      xs[k] = v, xs[nx + k] = v;
    }
  }
}

__device__ __forceinline__ float cfg_value(float g, float c, float u) { return __fmaf_rn(g, __fsub_rn(c, u), u); }

// head: the scalar elements in front of the first 16-byte boundary of c (u has the same phase); nv float4 behind them;
// the rest (< 4) scalar.  vec == 0: every element scalar.
__global__ __launch_bounds__(256) void k_cfg_combine(float* __restrict__ c, const float* __restrict__ u, float g, size_t n,
                                                     int head, size_t nv, int vec) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!vec) {
    for (size_t i = i0; i < n; i += stride) c[i] = cfg_value(g, c[i], u[i]);
    return;
  }
  float4* c4 = reinterpret_cast<float4*>(c + head);
  const float4* u4 = reinterpret_cast<const float4*>(u + head);
  for (size_t i = i0; i < nv; i += stride) {
    float4 a = c4[i];
    const float4 b = u4[i];
    a.x = cfg_value(g, a.x, b.x), a.y = cfg_value(g, a.y, b.y), a.z = cfg_value(g, a.z, b.z), a.w = cfg_value(g, a.w, b.w);
    c4[i] = a;
  }
  const size_t tail0 = (size_t)head + 4 * nv;  // the up to 3 + 3 scalar elements around the vector body
  if (i0 < (size_t)head) c[i0] = cfg_value(g, c[i0], u[i0]);
  if (i0 < n - tail0) c[tail0 + i0] = cfg_value(g, c[tail0 + i0], u[tail0 + i0]);
}

__global__ __launch_bounds__(256) void k_class_drop(const int32_t* __restrict__ labels, int n_classes,
                                                    const int64_t* __restrict__ index, int B, float p, uint64_t seed,
                                                    uint64_t sample_offset, int32_t* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t row = index ? (uint64_t)index[b] : (uint64_t)b;
  const uint64_t gi = sample_offset + row;  // slot gi & 3 of block gi >> 2, as k_sm_draw_times_at counts its rows
  const U4 ctr = {(uint32_t)(gi >> 2), (uint32_t)(gi >> 34), SM_TAG_CLASS_DROP, 0x46464446u};
  const U4 r = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int sl = (int)(gi & 3);
  const uint32_t w = sl == 0 ? r.x : sl == 1 ? r.y : sl == 2 ? r.z : r.w;
  const float uu = (float)(w >> 8) * (1.0f / 16777216.0f);  // [0, 1), exact
  out[b] = (uu < p || !labels) ? n_classes : labels[row];
}

__global__ __launch_bounds__(256) void k_class_table_grad(const float* __restrict__ dtemb, const int32_t* __restrict__ eff,
                                                          int n_classes, int B, int d, float* __restrict__ dtable) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (n_classes + 1) * d) return;
  const int cls = i / d, j = i - cls * d;
  double a = 0.0;
  for (int b = 0; b < B; ++b)
    if (class_row(eff, b, n_classes) == cls) a += (double)dtemb[(size_t)b * d + j];
  dtable[i] = (float)a;
}

static unsigned grid_for(size_t n) {
  const size_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : g > 65536 ? 65536 : g);
}

hipError_t launch_class_temb(const float* temb, int temb_stride, const float* table, int n_classes, const int32_t* labels,
                             int B, int d, int stack, float* out, const float* x, float* xs, size_t nx, hipStream_t s) {
  const int rows = stack ? 2 * B : B;
  hipLaunchKernelGGL(k_class_temb, dim3(grid_for((size_t)rows * d + (xs ? nx : 0))), dim3(256), 0, s, temb, temb_stride, table,
                     n_classes, labels, B, d, rows, out, x, xs, nx);
  return hipGetLastError();
}

hipError_t launch_cfg_combine(float* c, const float* u, float g, size_t n, hipStream_t s) {
  const uintptr_t pc = reinterpret_cast<uintptr_t>(c), pu = reinterpret_cast<uintptr_t>(u);
  // float4 where both pointers reach a 16-byte boundary after the same number of elements
  int vec = (pc & 15) == (pu & 15) && (pc & 3) == 0;
  int head = vec ? (int)(((16 - (pc & 15)) & 15) / 4) : 0;
  if ((size_t)head > n) head = (int)n;
  const size_t nv = vec ? (n - head) / 4 : 0;
  if (nv == 0) vec = 0, head = 0;
  hipLaunchKernelGGL(k_cfg_combine, dim3(grid_for(vec ? nv : n)), dim3(256), 0, s, c, u, g, n, head, nv, vec);
  return hipGetLastError();
}

hipError_t launch_class_drop(const int32_t* labels, int n_classes, const int64_t* index, int B, float p_uncond, uint64_t seed,
                             uint64_t sample_offset, int32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_class_drop, dim3(cdiv(B, 256)), dim3(256), 0, s, labels, n_classes, index, B, p_uncond, seed,
                     sample_offset, out);
  return hipGetLastError();
}

hipError_t launch_class_table_grad(const float* dtemb, const int32_t* eff_labels, int n_classes, int B, int d, float* dtable,
                                   hipStream_t s) {
  hipLaunchKernelGGL(k_class_table_grad, dim3(cdiv((n_classes + 1) * d, 256)), dim3(256), 0, s, dtemb, eff_labels, n_classes, B,
                     d, dtable);
  return hipGetLastError();
}

}  // namespace ffd

// ---- C ABI (include/ffd.h) ----
using namespace ffd;

extern "C" {

int ffd_class_temb(const float* temb, int temb_stride, const float* table, int n_classes, const int32_t* labels, int B, int d,
                   int stack, float* out, void* stream) {
  if (!temb || !table || !out || B < 1 || d < 1 || n_classes < 1) return FFD_ERR_INVALID;
  if (temb_stride != 0 && temb_stride != d) return FFD_ERR_INVALID;
  if (out == table || (out == temb && (temb_stride != d || stack))) return FFD_ERR_INVALID;
  if ((double)B * d * 2 >= 2147483648.0 || (double)(n_classes + 1) * d >= 2147483648.0) return FFD_ERR_UNSUPPORTED;
  return launch_class_temb(temb, temb_stride, table, n_classes, labels, B, d, stack ? 1 : 0, out, nullptr, nullptr, 0,
                           (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_cfg_combine(float* c, const float* u, float g, size_t n, void* stream) {
  if (!c || !u || c == u || n < 1 || !std::isfinite(g)) return FFD_ERR_INVALID;
  if (((reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(u)) & 3) != 0) return FFD_ERR_INVALID;
  return launch_cfg_combine(c, u, g, n, (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_class_drop(const int32_t* labels, int n_classes, const int64_t* index, int B, double p_uncond, uint64_t seed,
                   uint64_t sample_offset, int32_t* out, void* stream) {
  if (!out || B < 1 || n_classes < 1 || !(p_uncond >= 0.0 && p_uncond <= 1.0) || out == labels) return FFD_ERR_INVALID;
  return launch_class_drop(labels, n_classes, index, B, (float)p_uncond, seed, sample_offset, out, (hipStream_t)stream) ==
                 hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_class_table_grad(const float* dtemb, const int32_t* eff_labels, int n_classes, int B, int d, float* dtable,
                         void* stream) {
  if (!dtemb || !eff_labels || !dtable || B < 1 || d < 1 || n_classes < 1) return FFD_ERR_INVALID;
  if ((double)B * d >= 2147483648.0 || (double)(n_classes + 1) * d >= 2147483648.0) return FFD_ERR_UNSUPPORTED;
  return launch_class_table_grad(dtemb, eff_labels, n_classes, B, d, dtable, (hipStream_t)stream) == hipSuccess ? FFD_OK
                                                                                                                 : FFD_ERR_HIP;
}

}  // extern "C"
