// The pointwise step of the samplers on a (B, L, C) state: one grid-stride float4 kernel, one scalar kernel and one
// launcher for every update rule ("op") that works element by element with the row's G_l.  An op is a struct passed by
// value.  It holds its arrays and parameters and states
//   DRAWS   it takes one N(0,1) draw per element (its member `d`: injected z or Philox under d.tag)
//   SAMPLE  it needs the sample index b (skip(b): leave the sample as it is); the other ops do not pay the division
//   aligned()  its arrays allow float4 access
//   NIN, load<W>(i, in)  the arrays it reads for the W elements of float4 i (W = 4) or for element i (W = 1); the
//           kernel issues these loads first, so that they fly under the generator's arithmetic and the G_l load
//   update<W>(i, in, Gl, zz, b)  the update of those elements and its stores
// The draw of global element g is slot g & 3 of Philox block g >> 2 under the op's tag, whichever kernel asks.
#pragma once
#include "ffd_internal.h"

namespace ffd {

struct Draws {
  const float* z;  // injected draws, or nullptr: Philox (seed, tag) at global element elem_offset + i
  uint64_t seed, elem_offset;
  uint32_t tag;
};

// W consecutive floats: float4 i of p (W = 4) or element i (W = 1)
template <int W>
__device__ __forceinline__ void ld(const float* p, size_t i, float (&a)[W]) {
  if constexpr (W == 4) {
    const float4 v = reinterpret_cast<const float4*>(p)[i];
    a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
  } else {
    a[0] = p[i];
  }
}
template <int W>
__device__ __forceinline__ void st(float* p, size_t i, const float (&a)[W]) {
  if constexpr (W == 4) reinterpret_cast<float4*>(p)[i] = float4{a[0], a[1], a[2], a[3]};
  else p[i] = a[0];
}

// The probability-flow ODE's drift d(x, t) = f(x, t) - 1/2 (g(t) G_l)^2 s of one element (include/ffd.h ffd_ode_step),
// every product / sum its own fp32 rounding: the sampling tails (ffd_elem.hip) and the likelihood tail (ffd_loglik.hip)
__device__ __forceinline__ float ode_drift(float xi, float sc, float Gl, const SdeParams& p) {
  const float g = __fmul_rn(p.cs, Gl);
  const float g2 = __fmul_rn(g, g);
  const float gs = __fmul_rn(g2, sc);
  const float hgs = __fmul_rn(0.5f, gs);
  return (p.sde == 0) ? __fsub_rn(__fmul_rn(p.a, xi), hgs) : -hgs;
}

// C % 4 == 0, 16-byte aligned arrays, elem_offset % 4 == 0: one float4 per array, thread and iteration; the four
// elements share their row, so G[l] is one load, and their draws are one Philox block.
template <class Op>
__global__ __launch_bounds__(256) void k_step_v4(Op op, const float* __restrict__ G, size_t nvec, int L, unsigned C4) {
  const size_t per = (size_t)L * C4;  // float4 per sample
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    size_t b = 0;
    if constexpr (Op::SAMPLE) {
      b = v / per;
      if (op.skip(b)) continue;
    }
    float in[Op::NIN][4], zz[4] = {0.f, 0.f, 0.f, 0.f};
    op.template load<4>(v, in);
    if constexpr (Op::DRAWS) {
      if (op.d.z) ld<4>(op.d.z, v, zz);
      else normal4((op.d.elem_offset >> 2) + v, op.d.seed, op.d.tag, zz);
    }
    op.template update<4>(v, in, G[(v / C4) % (size_t)L], zz, b);
  }
}

// any C, any alignment: four elements per thread and iteration (whole Philox blocks where the offset allows)
template <class Op>
__global__ __launch_bounds__(256) void k_step(Op op, const float* __restrict__ G, size_t total, int L, int C) {
  const size_t nvec = (total + 3) / 4, per = (size_t)L * C;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    const size_t i0 = v * 4;
    const int n = (int)((total - i0) < 4 ? (total - i0) : 4);
    float zz[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (Op::DRAWS) load_normals(op.d.z, i0, n, op.d.seed, op.d.elem_offset, op.d.tag, zz);
    for (int j = 0; j < n; ++j) {
      const size_t i = i0 + j;
      size_t b = 0;
      if constexpr (Op::SAMPLE) {
        b = i / per;
        if (op.skip(b)) continue;
      }
      float in[Op::NIN][1];
      const float z1[1] = {zz[j]};
      op.template load<1>(i, in);
      op.template update<1>(i, in, G[(i / (size_t)C) % (size_t)L], z1, b);
    }
  }
}

// 256 threads, at most 4096 blocks; the float4 kernel where every array allows it
template <class Op>
hipError_t launch_step(Op op, const float* G, int B, int L, int C, hipStream_t s) {
  const size_t total = (size_t)B * L * C;
  size_t blocks = ((total + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  bool vec = C % 4 == 0 && op.aligned();
  if constexpr (Op::DRAWS) vec = vec && ptr16(op.d.z) && op.d.elem_offset % 4 == 0;
  if (vec) hipLaunchKernelGGL(k_step_v4<Op>, dim3((unsigned)blocks), dim3(256), 0, s, op, G, total / 4, L, (unsigned)C / 4);
  else hipLaunchKernelGGL(k_step<Op>, dim3((unsigned)blocks), dim3(256), 0, s, op, G, total, L, C);
  return hipGetLastError();
}

}  // namespace ffd
