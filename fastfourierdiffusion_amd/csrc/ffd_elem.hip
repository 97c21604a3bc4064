// Element-wise / small kernels of the sampling path (gfx950).
//   - weight packing into MFMA fragment order, nn.Embedding(max_norm) renorm
//   - Gaussian-Fourier time embedding, channel embed / unembed
//   - VP / VE reverse Euler-Maruyama step with on-device Philox4x32-10 noise
//   - probability-flow ODE intervals (Euler, Heun predictor / corrector): no noise draw
//   - linear multistep ODE intervals (Adams-Bashforth 2, DPM-Solver++ 2M): one operation, coefficients from the host
//   - KV-table store
// All HBM-bound: one pass over the data, coalesced, no re-reads.
// The entry points that need no context (SDE step, prior, the two encodings, Hermite prediction) follow the kernels.
#include <math.h>

#include <algorithm>

#include "ffd_step.h"

namespace ffd {

// ---------------------------------------------------------------------------
// packing
// ---------------------------------------------------------------------------
__global__ void k_pack_dweight(const float* __restrict__ W, float* __restrict__ Wp, int N, int D) {
  const int G = dpack_groups(D);
  const size_t total = dpack_floats(N, D);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int j = i & 3;
    int lane = (i >> 2) & 63;
    size_t rest = i >> 8;
    int g = rest % G;
    int nt = rest / G;
    int n = 16 * nt + (lane & 15);
    int k = 4 * (4 * g + j) + (lane >> 4);
    Wp[i] = (n < N && k < D) ? W[(size_t)n * D + k] : 0.f;
  }
}

__global__ void k_pack_w2(const float* __restrict__ W2, float* __restrict__ W2p, int D, int F) {
  const int CT = cdiv(D, 16);
  const size_t total = w2pack_floats(D, F);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int r = i & 3;
    int lane = (i >> 2) & 63;
    size_t rest = i >> 8;
    int ct = rest % CT;
    int fc = rest / CT;
    int c = 16 * ct + (lane & 15);
    int f = 16 * fc + 4 * (lane >> 4) + r;
    W2p[i] = (c < D) ? W2[(size_t)c * F + f] : 0.f;
  }
}

__global__ void k_pack_w2rem(const float* __restrict__ W2, float* __restrict__ W2r, int D, int F) {
  const int NG = w2rem_groups(D);
  const int c0 = 16 * (D / 16);
  const size_t total = (size_t)(F / 16) * NG * 64 * 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int r = i & 3;
    int lane = (i >> 2) & 63;
    size_t rest = i >> 8;
    int g = rest % NG;
    int fc = rest / NG;
    int c = c0 + 4 * g + (lane & 3);
    int f = 16 * fc + 4 * (lane >> 4) + r;
    W2r[i] = W2[(size_t)c * F + f];
  }
}

hipError_t launch_pack_w2rem(const float* W2, float* W2r, int D, int F, hipStream_t s) {
  if (w2rem_groups(D) == 0) return hipSuccess;
  size_t total = (size_t)(F / 16) * w2rem_groups(D) * 64 * 4;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_pack_w2rem, dim3(blocks), dim3(256), 0, s, W2, W2r, D, F);
  return hipGetLastError();
}

hipError_t launch_pack_dweight(const float* W, float* Wp, int N, int D, hipStream_t s) {
  size_t total = dpack_floats(N, D);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_pack_dweight, dim3(blocks), dim3(256), 0, s, W, Wp, N, D);
  return hipGetLastError();
}

hipError_t launch_pack_w2(const float* W2, float* W2p, int D, int F, hipStream_t s) {
  size_t total = w2pack_floats(D, F);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_pack_w2, dim3(blocks), dim3(256), 0, s, W2, W2p, D, F);
  return hipGetLastError();
}

// nn.Embedding(max_norm): rows with ||w|| > max_norm scaled by max_norm/(||w||+1e-7),
// iterated to the fixed point the reference reaches after a few lookups.
__global__ void k_renorm_rows(float* __restrict__ W, int D, float max_norm) {
  float* w = W + (size_t)blockIdx.x * D;
  __shared__ float red[WAVE];
  for (int it = 0; it < 8; ++it) {
    float ss = 0.f;
    for (int k = threadIdx.x; k < D; k += WAVE) ss += w[k] * w[k];
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    float norm = sqrtf(ss);
    if (!(norm > max_norm)) break;  // wave-uniform
    float scale = max_norm / (norm + 1e-7f);
    for (int k = threadIdx.x; k < D; k += WAVE) w[k] *= scale;
    __syncthreads();
  }
  (void)red;
}

hipError_t launch_renorm_rows(float* W, int rows, int D, float max_norm, hipStream_t s) {
  hipLaunchKernelGGL(k_renorm_rows, dim3(rows), dim3(WAVE), 0, s, W, D, max_norm);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// time embedding: temb[n][:] = dense([sin(2 pi t W), cos(2 pi t W)][:d])
// ---------------------------------------------------------------------------
__global__ void k_time_embed(const float* __restrict__ ts, float t_imm, const float* __restrict__ W,
                             const float* __restrict__ dw, const float* __restrict__ db, float* __restrict__ temb,
                             int D) {
  extern __shared__ float emb[];
  const float t = ts ? ts[blockIdx.x] : t_imm;
  const int half = (D + 1) / 2;
  for (int j = threadIdx.x; j < D; j += blockDim.x) {
    // ((t * W) * 2) * pi, each product rounded to fp32 (transformer.py:80)
    float w = W[j < half ? j : j - half];
    float proj = __fmul_rn(__fmul_rn(__fmul_rn(t, w), 2.0f), 3.14159265358979323846f);
    emb[j] = (j < half) ? sinf(proj) : cosf(proj);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < D; j += blockDim.x) {
    float acc = db[j];
    const float* row = dw + (size_t)j * D;
    for (int k = 0; k < D; ++k) acc = fmaf(emb[k], row[k], acc);
    temb[(size_t)blockIdx.x * D + j] = acc;
  }
}

hipError_t launch_time_embed(const float* ts, float t_imm, int n, const float* W, const float* dense_w,
                             const float* dense_b, float* temb, int D, hipStream_t s) {
  hipLaunchKernelGGL(k_time_embed, dim3(n), dim3(128), D * sizeof(float), s, ts, t_imm, W, dense_w, dense_b, temb, D);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// embed: h[row][j] = be[j] + sum_c X[row][c] We[j][c] (+ pos[l][j]) + temb[b][j]
// ---------------------------------------------------------------------------
// Write-bound (4 (C + D) bytes per row, D >> C).  k_embed_reg (C <= 8): a thread owns ONE (position l, float4 column
// j) of the output and walks the batch: its 4 x C embedder weights, bias, POSITIONAL float4 and (shared) time
// embedding stay in registers, so the loop body is the row's x (C floats, float4 loads when C % 4 == 0; the D/4
// threads of a row share them through L1), 4 C FMAs and one float4 store -- consecutive threads are consecutive
// float4 of consecutive rows, every wave writes one contiguous 1 KiB run.  No LDS, no table reads, no integer
// division in the loop; four samples per iteration keep four rows of loads in flight.
//
// LDSX: the D/4 threads of a row all need the same C floats of x.  As per-lane loads that is two 64-lane float4
// load instructions per stored KiB -- twice the address-path work of the store itself, and the kernel ran at 2.9 TB/s
// where its stores alone reach 6.1 (tools/probes/embed_sweep.py with the loads removed).  Instead the wave fetches the
// (<= 64) contiguous floats of x its 64 lanes' rows need with ONE dword load, parks them in LDS and every lane reads
// its row from there.  Slices are padded to whole waves so that the cooperating lanes share (slice, first row).
template <bool XVEC, bool LDSX, bool TS>
__global__ __launch_bounds__(256) void k_embed_reg(const float* __restrict__ X, const float* __restrict__ We,
                                                   const float* __restrict__ be, const float* __restrict__ pos,
                                                   const float* __restrict__ temb, int temb_stride,
                                                   float* __restrict__ h, int B, int L, int C, int D, int nslices) {
  __shared__ __align__(16) float xsh[LDSX ? 4 * 8 * 64 : 4];  // [wave][2 groups x 4 samples][float of the wave's x rows]
  const unsigned D4 = (unsigned)D >> 2;
  const unsigned LJ = (unsigned)L * D4;
  const unsigned LJP = LDSX ? (LJ + 63u) & ~63u : LJ;  // threads per slice
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned slice = g / LJP;
  if (slice >= (unsigned)nslices) return;
  const unsigned ljr = g - slice * LJP;
  const bool active = ljr < LJ;                    // (LDSX: the pad lanes of a slice's last wave help load, never store)
  const unsigned lj = active ? ljr : LJ - 1;
  const unsigned l = lj / D4;
  const int j = (int)(lj - l * D4) << 2;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned r0 = (ljr - lane) / D4;           // first row of this wave
  const unsigned rl = min(ljr - lane + 63u, LJ - 1) / D4;
  const unsigned nf = (rl - r0 + 1) * (unsigned)C;  // floats of x the wave needs per sample (<= 64, launcher)
  const unsigned rel = (l - r0) * (unsigned)C;
  float* xw = xsh + (LDSX ? (threadIdx.x >> 6) * 512 : 0);
  float4 w[8];
  if (XVEC) {  // C = 4 or 8: the four weight rows j .. j+3 as float4 loads (8 instead of 32 per thread)
    float wr[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 a = *reinterpret_cast<const float4*>(We + (size_t)(j + k) * C);
      const float4 a2 = C > 4 ? *reinterpret_cast<const float4*>(We + (size_t)(j + k) * C + 4) : float4{0.f, 0.f, 0.f, 0.f};
      wr[k][0] = a.x, wr[k][1] = a.y, wr[k][2] = a.z, wr[k][3] = a.w;
      wr[k][4] = a2.x, wr[k][5] = a2.y, wr[k][6] = a2.z, wr[k][7] = a2.w;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = float4{wr[0][c], wr[1][c], wr[2][c], wr[3][c]};
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      w[c] = c < C ? float4{We[(j + 0) * C + c], We[(j + 1) * C + c], We[(j + 2) * C + c], We[(j + 3) * C + c]}
                   : float4{0.f, 0.f, 0.f, 0.f};
  }
  const float4 bias = *reinterpret_cast<const float4*>(be + j);
  const float4 p = pos ? *reinterpret_cast<const float4*>(pos + (size_t)l * D + j) : float4{0.f, 0.f, 0.f, 0.f};
  const float4 t0 = *reinterpret_cast<const float4*>(temb + j);  // the shared time embedding (temb_stride == 0)
  auto fetch_x = [&](int b, int u) {  // LDSX: the wave's x floats of sample b -> LDS slot u
    if (lane < nf) xw[u * 64 + lane] = X[((size_t)b * L + r0) * C + lane];
  };
  auto load_x = [&](int b, int u, float (&xv)[8]) {
    const float* x = LDSX ? xw + u * 64 + rel : X + ((size_t)b * L + l) * C;
    if (XVEC) {
      const float4 a = *reinterpret_cast<const float4*>(x);
      xv[0] = a.x, xv[1] = a.y, xv[2] = a.z, xv[3] = a.w;
      if (C > 4) {
        const float4 a2 = *reinterpret_cast<const float4*>(x + 4);
        xv[4] = a2.x, xv[5] = a2.y, xv[6] = a2.z, xv[7] = a2.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) xv[c] = c < C ? x[c] : 0.f;
    }
  };
  auto emit = [&](int b, const float (&xv)[8]) {
    float4 v = bias;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < C) v.x = fmaf(xv[c], w[c].x, v.x), v.y = fmaf(xv[c], w[c].y, v.y), v.z = fmaf(xv[c], w[c].z, v.z), v.w = fmaf(xv[c], w[c].w, v.w);
    if (pos) v.x += p.x, v.y += p.y, v.z += p.z, v.w += p.w;
    // (TS at compile time: as `temb_stride ? *p : t0` hipcc selected between the two ADDRESSES -- t0 parked in scratch,
    //  32 B per lane, and a flat load per stored float4 even where the batch shares one time embedding)
    float4 t = t0;
    if constexpr (TS) t = *reinterpret_cast<const float4*>(temb + (size_t)b * temb_stride + j);
    if (active) *reinterpret_cast<float4*>(h + ((size_t)b * L + l) * D + j) = float4{v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w};
  };
  int b = (int)slice;
  int grp = 0;  // LDSX: which half of the wave's LDS slots holds the current group of four samples
  if (LDSX && b + 3 * nslices < B) {
#pragma unroll
    for (int u = 0; u < 4; ++u) fetch_x(b + u * nslices, u);
  }
  for (; b + 3 * nslices < B; b += 4 * nslices) {
    float xa[4][8];
    if (LDSX) {  // the next group's x is requested before this group is consumed (the loop is latency-bound otherwise)
      if (b + 7 * nslices < B) {
#pragma unroll
        for (int u = 0; u < 4; ++u) fetch_x(b + (4 + u) * nslices, 4 * (grp ^ 1) + u);
      }
      __builtin_amdgcn_wave_barrier();  // (one wave, in-order LDS: only the compiler must keep the order)
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) load_x(b + u * nslices, 4 * grp + u, xa[u]);
    if (LDSX) __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < 4; ++u) emit(b + u * nslices, xa[u]);
    grp ^= 1;
  }
  for (; b < B; b += nslices) {
    float xa[8];
    if (LDSX) {
      fetch_x(b, 0);
      __builtin_amdgcn_wave_barrier();
    }
    load_x(b, 0, xa);
    if (LDSX) __builtin_amdgcn_wave_barrier();
    emit(b, xa);
  }
}

__global__ void k_embed(const float* __restrict__ X, const float* __restrict__ We, const float* __restrict__ be,
                        const float* __restrict__ pos, const float* __restrict__ temb, int temb_stride,
                        float* __restrict__ h, unsigned total4, int L, int C, int D) {
  // generic C: the (D x C) embedder weight is staged transposed in LDS ([c][j]); one float4 of h per thread and
  // iteration (D % 4 == 0); same operation order as k_embed_reg.
  extern __shared__ __align__(16) float wt[];  // C * D floats
  for (int i = threadIdx.x; i < C * D; i += blockDim.x) {
    const int c = i / D, j = i - c * D;
    wt[i] = We[j * C + c];
  }
  __syncthreads();
  for (unsigned i4 = blockIdx.x * blockDim.x + threadIdx.x; i4 < total4; i4 += gridDim.x * blockDim.x) {
    const unsigned row = (4u * i4) / (unsigned)D;
    const int j = (int)(4u * i4 - row * (unsigned)D);
    const unsigned bidx = row / (unsigned)L;
    const int l = (int)(row - bidx * (unsigned)L);
    const float* x = X + (size_t)row * C;
    float4 v = float4{be[j], be[j + 1], be[j + 2], be[j + 3]};
    for (int c = 0; c < C; ++c) {
      const float xc = x[c];
      const float4 w4 = *reinterpret_cast<const float4*>(&wt[c * D + j]);
      v.x = fmaf(xc, w4.x, v.x), v.y = fmaf(xc, w4.y, v.y), v.z = fmaf(xc, w4.z, v.z), v.w = fmaf(xc, w4.w, v.w);
    }
    if (pos) {
      const float4 p = *reinterpret_cast<const float4*>(pos + (size_t)l * D + j);
      v.x += p.x, v.y += p.y, v.z += p.z, v.w += p.w;
    }
    const float4 t = *reinterpret_cast<const float4*>(temb + (size_t)bidx * temb_stride + j);
    reinterpret_cast<float4*>(h)[i4] = float4{v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w};
  }
}


hipError_t launch_embed(const float* X, const float* We, const float* be, const float* pos, const float* temb,
                        int temb_stride, float* h, int B, int L, int C, int D, hipStream_t s) {
  const unsigned M = (unsigned)B * (unsigned)L;
  const unsigned total4 = (unsigned)((size_t)M * D / 4);
  if (C <= 8 && D % 4 == 0) {
    // one thread per (l, float4 column) and batch slice: as many slices as give ~512 k threads
    const unsigned D4 = (unsigned)(D / 4);
    const unsigned LJ = (unsigned)L * D4;
    // x through LDS when the rows of 64 consecutive lanes (64 / D4, + 2 for a wave that starts and ends mid-row)
    // need at most 64 floats of x
    // (only where it replaces float4 loads, C = 4 or 8: with one float per row the detour costs more than it saves)
    const bool ldsx = g_embed_ldsx && (C == 4 || C == 8) && (64u / D4 + 2u) * (unsigned)C <= 64u;
    const unsigned LJP = ldsx ? (LJ + 63u) & ~63u : LJ;
    int nslices = (int)((unsigned)g_embed_threads / LJP);
    if (nslices < 1) nslices = 1;
    if (nslices > B) nslices = B;
    const unsigned blocks = (unsigned)(((size_t)nslices * LJP + 255) / 256);
    const bool xvec = (C == 4 || C == 8) && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(We)) & 15) == 0;
#define FFD_EMBED(xv, lx)                                                                                              \
  do {                                                                                                                 \
    if (temb_stride)                                                                                                   \
      hipLaunchKernelGGL((k_embed_reg<xv, lx, true>), dim3(blocks), dim3(256), 0, s, X, We, be, pos, temb, temb_stride, h, B, L, C, D, nslices); \
    else                                                                                                               \
      hipLaunchKernelGGL((k_embed_reg<xv, lx, false>), dim3(blocks), dim3(256), 0, s, X, We, be, pos, temb, temb_stride, h, B, L, C, D, nslices); \
  } while (0)
    if (xvec && ldsx) FFD_EMBED(true, true);
    else if (xvec) FFD_EMBED(true, false);
    else if (ldsx) FFD_EMBED(false, true);
    else FFD_EMBED(false, false);
#undef FFD_EMBED
    return hipGetLastError();
  }
  unsigned blocks = (total4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;  // grid-stride: the weight staging is amortised over >= a few rows per thread
  const size_t lds = (size_t)C * D * sizeof(float);
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_embed, dim3(blocks), dim3(256), lds, s, X, We, be, pos, temb, temb_stride, h, total4, L, C, D);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// standalone encoders: out[b,l,:] = x[b,l,:] + rowtab[l,:] (positional) or + battab[b,:] (time)
// ---------------------------------------------------------------------------
__global__ void k_add_table(const float* __restrict__ x, const float* __restrict__ rowtab,
                            const float* __restrict__ battab, float* __restrict__ out, unsigned total, int L, int D) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned row = i / (unsigned)D;
    const int j = (int)(i - row * (unsigned)D);
    const unsigned b = row / (unsigned)L;
    const int l = (int)(row - b * (unsigned)L);
    float v = x[i];
    if (rowtab) v += rowtab[(size_t)l * D + j];
    if (battab) v += battab[(size_t)b * D + j];
    out[i] = v;
  }
}

static hipError_t launch_add_table(const float* x, const float* rowtab, const float* battab, float* out, int B, int L, int D,
                                   hipStream_t s) {
  const unsigned total = (unsigned)((size_t)B * L * D);
  unsigned blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_add_table, dim3(blocks), dim3(256), 0, s, x, rowtab, battab, out, total, L, D);
  return hipGetLastError();
}

// one nn.Embedding(max_norm) lookup-time renormalisation pass (torch embedding_renorm_)
__global__ void k_renorm_rows_once(float* __restrict__ W, int D, float max_norm) {
  float* w = W + (size_t)blockIdx.x * D;
  float ss = 0.f;
  for (int k = threadIdx.x; k < D; k += WAVE) ss += w[k] * w[k];
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  const float norm = sqrtf(ss);
  if (norm > max_norm) {
    const float scale = max_norm / (norm + 1e-7f);
    for (int k = threadIdx.x; k < D; k += WAVE) w[k] *= scale;
  }
}

static hipError_t launch_renorm_rows_once(float* W, int rows, int D, float max_norm, hipStream_t s) {
  hipLaunchKernelGGL(k_renorm_rows_once, dim3(rows), dim3(WAVE), 0, s, W, D, max_norm);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// reverse SDE step (sde.py:129-165, 215-246), elementwise form of the reference's
// diag(L x L) matmuls.  No FMA contraction: each product / sum rounds like the
// reference's separate torch ops.
//   VP: drift = a*x - (g*g)*s ;  x' = (x - drift*dt) + sqdt*(g*z),  g = cs*G[l]
//   VE: drift = -((g*g)*s)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float sde_update(float xi, float sc, float Gl, float zz, const SdeParams& p) {
  const float g = __fmul_rn(p.cs, Gl);
  const float g2 = __fmul_rn(g, g);
  const float gs = __fmul_rn(g2, sc);
  const float drift = (p.sde == 0) ? __fsub_rn(__fmul_rn(p.a, xi), gs) : -gs;
  const float t1 = __fsub_rn(xi, __fmul_rn(drift, p.dt));
  return __fadd_rn(t1, __fmul_rn(p.sqdt, __fmul_rn(g, zz)));
}

// The stand-alone step kernels are k_step_v4<Op> / k_step<Op> (ffd_step.h) on the ops below.  12 B per element.
struct OpSde {
  static constexpr bool DRAWS = true, SAMPLE = false;
  float* x;
  const float* score;
  SdeParams p;
  Draws d;
  static constexpr int NIN = 2;  // x, score
  bool aligned() const { return ptr16(x) && ptr16(score); }
  template <int W>
  __device__ void load(size_t i, float (&in)[NIN][W]) const {
    ld<W>(x, i, in[0]), ld<W>(score, i, in[1]);
  }
  template <int W>
  __device__ void update(size_t i, float (&in)[NIN][W], float Gl, const float (&zz)[W], size_t) const {
#pragma unroll
    for (int j = 0; j < W; ++j) in[0][j] = sde_update(in[0][j], in[1][j], Gl, zz[j], p);
    st<W>(x, i, in[0]);
  }
};

hipError_t launch_sde_step(float* x, const float* score, const float* z, const float* G, SdeParams p, uint64_t seed,
                           uint64_t elem_offset, uint32_t step, int B, int L, int C, hipStream_t s) {
  return launch_step(OpSde{x, score, p, Draws{z, seed, elem_offset, step}}, G, B, L, C, s);
}

// ---------------------------------------------------------------------------
// Conditional sampling by replacement, time-domain models (include/ffd.h ffd_cond_project, FFD_COND_TIME): pointwise
//   y = (mc obs) + ((sigma G_l) z)   (noiseless: y = obs);   x <- x + mask (y - x)
// every product / sum its own fp32 rounding; the draws are counted like the SDE step's (OpSde).
// ---------------------------------------------------------------------------
__global__ void k_cond_time(float* __restrict__ x, const float* __restrict__ obs, const float* __restrict__ mask,
                            const float* __restrict__ z, const float* __restrict__ G, float mc, float sigma, int noiseless,
                            uint64_t seed, uint64_t elem_offset, uint32_t tag, int shared_obs, size_t total, int L, int C) {
  const size_t nvec = (total + 3) / 4, per = (size_t)L * C;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    const size_t i0 = v * 4;
    const int n = (int)((total - i0) < 4 ? (total - i0) : 4);
    float zz[4] = {0.f, 0.f, 0.f, 0.f};
    if (!noiseless) load_normals(z, i0, n, seed, elem_offset, tag, zz);
    for (int j = 0; j < n; ++j) {
      const size_t i = i0 + j;
      const size_t io = shared_obs ? i % per : i;
      float y = obs[io];
      if (!noiseless) {
        const float Gl = G[(i / (size_t)C) % (size_t)L];
        y = __fadd_rn(__fmul_rn(mc, y), __fmul_rn(__fmul_rn(sigma, Gl), zz[j]));
      }
      const float xi = x[i];
      x[i] = __fadd_rn(xi, __fmul_rn(mask[io], __fsub_rn(y, xi)));
    }
  }
}

hipError_t launch_cond_time(float* x, const float* obs, const float* mask, const float* G, float mc, float sigma,
                            int noiseless, const float* z, uint64_t seed, uint64_t elem_offset, uint32_t tag, int obs_batch,
                            int B, int L, int C, hipStream_t s) {
  const size_t total = (size_t)B * L * C;
  size_t blocks = ((total + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_cond_time, dim3((unsigned)blocks), dim3(256), 0, s, x, obs, mask, noiseless ? nullptr : z, G, mc,
                     sigma, noiseless, seed, elem_offset, tag, (int)(obs_batch == 1 && B > 1), total, L, C);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Forward transition of the SDE from time s to t >= s (include/ffd.h ffd_forward_transition; the re-noising of resampled
// conditional sampling):  x' = (a x) + ((sg G_l) z), every product / sum its own fp32 rounding; the draws are counted
// like the SDE step's.  noisy == 0 (sg == 0): x' = a x and no draw is read or generated.  8 B per element with device
// draws, 12 B with injected ones.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float transition_update(float xi, float Gl, float zz, float a, float sg, int noisy) {
  const float ax = __fmul_rn(a, xi);
  return noisy ? __fadd_rn(ax, __fmul_rn(__fmul_rn(sg, Gl), zz)) : ax;
}

// NOISY = false is there for callers of launch_forward_transition alone: transition_coef never gives an fp32 sg == 0
// with a != 1, so neither ffd_forward_transition nor the loop reaches it.
template <bool NOISY>
struct OpTransition {
  static constexpr bool DRAWS = NOISY, SAMPLE = false;
  float* x;
  float a, sg;
  Draws d;  // (NOISY)
  static constexpr int NIN = 1;  // x
  bool aligned() const { return ptr16(x); }
  template <int W>
  __device__ void load(size_t i, float (&in)[NIN][W]) const {
    ld<W>(x, i, in[0]);
  }
  template <int W>
  __device__ void update(size_t i, float (&in)[NIN][W], float Gl, const float (&zz)[W], size_t) const {
#pragma unroll
    for (int j = 0; j < W; ++j) in[0][j] = transition_update(in[0][j], Gl, zz[j], a, sg, NOISY);
    st<W>(x, i, in[0]);
  }
};

hipError_t launch_forward_transition(float* x, const float* G, float a, float sg, const float* z, uint64_t seed,
                                     uint64_t elem_offset, uint32_t tag, int B, int L, int C, hipStream_t s) {
  if (sg != 0.f) return launch_step(OpTransition<true>{x, a, sg, Draws{z, seed, elem_offset, tag}}, G, B, L, C, s);
  if (a == 1.f) return hipSuccess;  // s == t: x is untouched bit for bit (a x + 0 would turn -0 into +0)
  return launch_step(OpTransition<false>{x, a, sg, Draws{}}, G, B, L, C, s);
}

// ---------------------------------------------------------------------------
// probability-flow ODE steps (an extension: the reference has Euler-Maruyama only).  Same grid, G, beta(t) and VE
// sqrt_derivative as the SDE step (sde_params); the drift of the ODE with the SDE's marginals is
//   d(x, t) = f(x, t) - 1/2 (g(t) G_l)^2 s(x, t),   f = a*x (VP), 0 (VE)
// and one interval of width dt towards smaller t is
//   Euler:  x <- x - d(x, t_i) dt
//   Heun :  d1 = d(x, t_i);  xp = x - d1 dt;  d2 = d(xp, t_{i+1});  x <- x - (1/2 (d1 + d2)) dt
// No noise draw.  Like sde_update every product / sum is its own fp32 rounding (no FMA contraction).
// (ode_drift: ffd_step.h, shared with the likelihood tail of ffd_loglik.hip)
// ---------------------------------------------------------------------------
// One element of a tail.  EULER: returns the new x (xi = x).  PREDICT: returns xp, d1 = the drift at (x, t_i).
// CORRECT: xi = xp, sc = the score at xp, p = the parameters at t_{i+1}; x0 / d1 = what PREDICT read / wrote; returns
// the new x.
template <int TAIL>
__device__ __forceinline__ float ode_update(float xi, float sc, float Gl, float x0, float& d1, const SdeParams& p) {
  const float d = ode_drift(xi, sc, Gl, p);
  if (TAIL == ODE_CORRECT) return __fsub_rn(x0, __fmul_rn(__fmul_rn(0.5f, __fadd_rn(d1, d)), p.dt));
  if (TAIL == ODE_PREDICT) d1 = d;
  return __fsub_rn(xi, __fmul_rn(d, p.dt));
}

// Buffers by tail:
//   EULER    x in / out
//   PREDICT  x in, xp out, d1 out
//   CORRECT  xp in (score = the score at xp), x in / out, d1 in
template <int TAIL>
struct OpOde {
  static constexpr bool DRAWS = false, SAMPLE = false;
  float* x;
  const float* score;
  float *xp, *d1;
  SdeParams p;
  static constexpr int NIN = 4;  // what ode_update starts from (x; CORRECT: xp), score, CORRECT's x and d1
  bool aligned() const { return ptr16(x) && ptr16(score) && ptr16(xp) && ptr16(d1); }
  template <int W>
  __device__ void load(size_t i, float (&in)[NIN][W]) const {
    ld<W>(TAIL == ODE_CORRECT ? xp : x, i, in[0]), ld<W>(score, i, in[1]);
    if (TAIL == ODE_CORRECT) ld<W>(x, i, in[2]), ld<W>(d1, i, in[3]);
  }
  template <int W>
  __device__ void update(size_t i, float (&in)[NIN][W], float Gl, const float (&)[W], size_t) const {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if (TAIL != ODE_CORRECT) in[2][j] = in[3][j] = 0.f;
      in[0][j] = ode_update<TAIL>(in[0][j], in[1][j], Gl, in[2][j], in[3][j], p);
    }
    st<W>(TAIL == ODE_PREDICT ? xp : x, i, in[0]);
    if (TAIL == ODE_PREDICT) st<W>(d1, i, in[3]);
  }
};

hipError_t launch_ode_step(int tail, float* x, const float* score, float* xp, float* d1, const float* G, SdeParams p,
                           int B, int L, int C, hipStream_t s) {
  switch (tail) {
    case ODE_EULER: return launch_step(OpOde<ODE_EULER>{x, score, nullptr, nullptr, p}, G, B, L, C, s);
    case ODE_PREDICT: return launch_step(OpOde<ODE_PREDICT>{x, score, xp, d1, p}, G, B, L, C, s);
    case ODE_CORRECT: return launch_step(OpOde<ODE_CORRECT>{x, score, xp, d1, p}, G, B, L, C, s);
    default: return hipErrorInvalidValue;
  }
}

// ---------------------------------------------------------------------------
// linear multistep ODE steps (Adams-Bashforth 2 on the drift above; DPM-Solver++ 2M on the data prediction): second
// order at one score evaluation per interval.  Both are this one operation (include/ffd.h ffd_ode_multistep_step); the
// five coefficients come from the host (multistep_coef):
//   q = qa x + qb G_l^2 s;   x <- x + (cxm1 x + cn q + cp q_prev);   hist <- q
// PREV = false is a trajectory's first interval: cp = 0 and hist is not read.  Every product / sum is its own fp32
// rounding, like ode_update.
// ---------------------------------------------------------------------------
template <bool PREV>
__device__ __forceinline__ float multistep_update(float xi, float sc, float Gl, float& hq, const MultistepParams& p) {
  const float g2 = __fmul_rn(Gl, Gl);
  const float u = __fmul_rn(g2, sc);
  const float q = __fadd_rn(__fmul_rn(p.qa, xi), __fmul_rn(p.qb, u));
  float inc = __fadd_rn(__fmul_rn(p.cxm1, xi), __fmul_rn(p.cn, q));
  if (PREV) inc = __fadd_rn(inc, __fmul_rn(p.cp, hq));
  hq = q;
  return __fadd_rn(xi, inc);
}

// x and hist in / out (PREV = false: hist out only)
template <bool PREV>
struct OpMultistep {
  static constexpr bool DRAWS = false, SAMPLE = false;
  float* x;
  const float* score;
  float* hist;
  MultistepParams p;
  static constexpr int NIN = 3;  // x, score, hist
  bool aligned() const { return ptr16(x) && ptr16(score) && ptr16(hist); }
  template <int W>
  __device__ void load(size_t i, float (&in)[NIN][W]) const {
    ld<W>(x, i, in[0]), ld<W>(score, i, in[1]);
    if (PREV) ld<W>(hist, i, in[2]);
  }
  template <int W>
  __device__ void update(size_t i, float (&in)[NIN][W], float Gl, const float (&)[W], size_t) const {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if (!PREV) in[2][j] = 0.f;
      in[0][j] = multistep_update<PREV>(in[0][j], in[1][j], Gl, in[2][j], p);
    }
    st<W>(x, i, in[0]), st<W>(hist, i, in[2]);
  }
};

hipError_t launch_multistep_step(float* x, const float* score, float* hist, const float* G, MultistepParams p,
                                 int have_prev, int B, int L, int C, hipStream_t s) {
  if (have_prev) return launch_step(OpMultistep<true>{x, score, hist, p}, G, B, L, C, s);
  return launch_step(OpMultistep<false>{x, score, hist, p}, G, B, L, C, s);
}

// prior: x = G (.) z  (VE: * sigma_max), sde.py:79-87,125-127
__device__ __forceinline__ float prior_value(float Gl, float zz, float scale) {
  const float v0 = __fmul_rn(Gl, zz);
  return (scale == 1.0f) ? v0 : __fmul_rn(scale, v0);
}

struct OpPrior {
  static constexpr bool DRAWS = true, SAMPLE = false;
  float* x;
  float scale;
  Draws d;
  static constexpr int NIN = 1;  // (nothing is read)
  bool aligned() const { return ptr16(x); }
  template <int W>
  __device__ void load(size_t, float (&)[NIN][W]) const {}
  template <int W>
  __device__ void update(size_t i, float (&in)[NIN][W], float Gl, const float (&zz)[W], size_t) const {
#pragma unroll
    for (int j = 0; j < W; ++j) in[0][j] = prior_value(Gl, zz[j], scale);
    st<W>(x, i, in[0]);
  }
};

static hipError_t launch_prior(float* x, const float* z, const float* G, float scale, uint64_t seed, uint64_t elem_offset,
                               int B, int L, int C, hipStream_t s) {
  return launch_step(OpPrior{x, scale, Draws{z, seed, elem_offset, 0xFFFFFFFFu}}, G, B, L, C, s);
}

// ---------------------------------------------------------------------------
// unembed: score[row][c] = bu[c] + h[row][:] . Wu[c][:]     (score_models.py:113)
// and, fused, a sampler's update of x on that score (the score never reaches HBM).
// ---------------------------------------------------------------------------
// HBM-bound on the read of h (4 D bytes per row against 4 C written).  One wave owns 16 rows per iteration and forms
// score^T (C x 16) on the exact-fp32 matrix core: A = the unembedder weight (channel on the row index, rows >= C
// zero), B = the h rows, each lane loading FOUR consecutive k of its row as one float4 per 16-wide k chunk (the
// MFMA's k index is then a permutation of the chunk's 16 k values, the same for A and B; the qkv kernel's trick).
// The accumulator leaves lane l with channels 4 (l >> 4) .. +3 of row (l & 15): exactly one float4 of score / x
// when C % 4 == 0.  The next tile's h is prefetched under the current tile's MFMAs and epilogue.
//
// What happens to the score quad is the Tail's, a struct passed by value with its arrays and parameters:
//   Regs                      the operand quads it wants fetched together with a tile's h rows (may be empty)
//   NEEDS_G                   whether it reads G[row % L]
//   load(i0, regs)            fetch them for the quad at element i0 (C % 4 == 0 only)
//   quad(i0, acc, Gl, regs)   C % 4 == 0: the update of the float4 at i0
//   ragged(i0, n, acc, Gl)    otherwise: the update of elements i0 .. i0 + n - 1, operands from HBM
// The tails use the update functions and the Philox indexing of the stand-alone ops above, so fused and unfused steps
// agree bit for bit.
struct TailStore {  // score <- unembed(h)
  struct Regs {};
  static constexpr bool NEEDS_G = false;
  float* score;
  __device__ void load(size_t, Regs&) const {}
  __device__ void quad(size_t i0, f32x4 acc, float, const Regs&) const {
    *reinterpret_cast<float4*>(score + i0) = float4{acc[0], acc[1], acc[2], acc[3]};
  }
  __device__ void ragged(size_t i0, int n, f32x4 acc, float) const {
    for (int i = 0; i < n; ++i) score[i0 + i] = acc[i];
  }
};

struct TailSde {  // Euler-Maruyama (OpSde)
  struct Regs { float4 x, z; };
  static constexpr bool NEEDS_G = true;
  float* x;
  SdeParams p;
  Draws d;
  __device__ void load(size_t i0, Regs& u) const {
    u.x = *reinterpret_cast<const float4*>(x + i0);
    if (d.z) u.z = *reinterpret_cast<const float4*>(d.z + i0);
  }
  __device__ void quad(size_t i0, f32x4 acc, float Gl, const Regs& u) const {
    float zz[4];
    if (d.z) zz[0] = u.z.x, zz[1] = u.z.y, zz[2] = u.z.z, zz[3] = u.z.w;
    else normal4((d.elem_offset + i0) >> 2, d.seed, d.tag, zz);
    *reinterpret_cast<float4*>(x + i0) = float4{sde_update(u.x.x, acc[0], Gl, zz[0], p), sde_update(u.x.y, acc[1], Gl, zz[1], p),
                                                sde_update(u.x.z, acc[2], Gl, zz[2], p), sde_update(u.x.w, acc[3], Gl, zz[3], p)};
  }
  __device__ void ragged(size_t i0, int n, f32x4 acc, float Gl) const {
    float zz[4];
    load_normals(d.z, i0, n, d.seed, d.elem_offset, d.tag, zz);
    for (int i = 0; i < n; ++i) x[i0 + i] = sde_update(x[i0 + i], acc[i], Gl, zz[i], p);
  }
};

template <int TAIL>
struct TailOde {  // OpOde<TAIL>; u0 = the quad ode_update starts from (x; CORRECT: xp), u1 / u2 = CORRECT's x and d1
  struct Regs { float4 u0, u1, u2; };
  static constexpr bool NEEDS_G = true;
  float *x, *xp, *d1;
  SdeParams p;
  __device__ void load(size_t i0, Regs& u) const {
    u.u0 = *reinterpret_cast<const float4*>((TAIL == ODE_CORRECT ? xp : x) + i0);
    if (TAIL == ODE_CORRECT) {
      u.u1 = *reinterpret_cast<const float4*>(x + i0);
      u.u2 = *reinterpret_cast<const float4*>(d1 + i0);
    }
  }
  __device__ void quad(size_t i0, f32x4 acc, float Gl, const Regs& u) const {
    float4 dv = u.u2;
    const float4 xn = float4{ode_update<TAIL>(u.u0.x, acc[0], Gl, u.u1.x, dv.x, p), ode_update<TAIL>(u.u0.y, acc[1], Gl, u.u1.y, dv.y, p),
                             ode_update<TAIL>(u.u0.z, acc[2], Gl, u.u1.z, dv.z, p), ode_update<TAIL>(u.u0.w, acc[3], Gl, u.u1.w, dv.w, p)};
    *reinterpret_cast<float4*>((TAIL == ODE_PREDICT ? xp : x) + i0) = xn;
    if (TAIL == ODE_PREDICT) *reinterpret_cast<float4*>(d1 + i0) = dv;
  }
  __device__ void ragged(size_t i0, int n, f32x4 acc, float Gl) const {
    for (int i = 0; i < n; ++i) {
      float dv = TAIL == ODE_CORRECT ? d1[i0 + i] : 0.f;
      const float x0 = TAIL == ODE_CORRECT ? x[i0 + i] : 0.f;
      const float xn = ode_update<TAIL>((TAIL == ODE_CORRECT ? xp : x)[i0 + i], acc[i], Gl, x0, dv, p);
      (TAIL == ODE_PREDICT ? xp : x)[i0 + i] = xn;
      if (TAIL == ODE_PREDICT) d1[i0 + i] = dv;
    }
  }
};

template <bool PREV>
struct TailMultistep {  // OpMultistep<PREV>; moves two (B, L, C) arrays more than Euler's: 4 (d + 4 C) B per row
  struct Regs { float4 x, hist; };
  static constexpr bool NEEDS_G = true;
  float *x, *hist;
  MultistepParams p;
  __device__ void load(size_t i0, Regs& u) const {
    u.x = *reinterpret_cast<const float4*>(x + i0);
    if (PREV) u.hist = *reinterpret_cast<const float4*>(hist + i0);
  }
  __device__ void quad(size_t i0, f32x4 acc, float Gl, const Regs& u) const {
    float4 hq = u.hist;
    *reinterpret_cast<float4*>(x + i0) =
        float4{multistep_update<PREV>(u.x.x, acc[0], Gl, hq.x, p), multistep_update<PREV>(u.x.y, acc[1], Gl, hq.y, p),
               multistep_update<PREV>(u.x.z, acc[2], Gl, hq.z, p), multistep_update<PREV>(u.x.w, acc[3], Gl, hq.w, p)};
    *reinterpret_cast<float4*>(hist + i0) = hq;
  }
  __device__ void ragged(size_t i0, int n, f32x4 acc, float Gl) const {
    for (int i = 0; i < n; ++i) {
      float hq = PREV ? hist[i0 + i] : 0.f;
      x[i0 + i] = multistep_update<PREV>(x[i0 + i], acc[i], Gl, hq, p);
      hist[i0 + i] = hq;
    }
  }
};

template <int D, class Tail>
__global__ __launch_bounds__(256) void k_unembed_mfma(const float* __restrict__ h, const float* __restrict__ Wu,
                                                      const float* __restrict__ bu, const float* __restrict__ G, Tail tail,
                                                      int M, int L, int C) {
  constexpr int NG = (D + 15) / 16;  // 16-wide k chunks
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int ntiles = (M + 15) >> 4;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  float4 wf[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int k = 16 * g + 4 * q;
    wf[g] = (r < C && k < D) ? *reinterpret_cast<const float4*>(Wu + (size_t)r * D + k) : float4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 bias;
#pragma unroll
  for (int i = 0; i < 4; ++i) bias[i] = (4 * q + i < C) ? bu[4 * q + i] : 0.f;
  // a tile's h rows and, where the lane holds a whole quad (C % 4 == 0), the tail's operands
  const bool quad = (C & 3) == 0 && 4 * q < C;
  auto load_tile = [&](int t, float4 (&hv)[NG], typename Tail::Regs& u) {
    const int row = min(16 * t + r, M - 1);
    const float* hr = h + (size_t)row * D + 4 * q;
#pragma unroll
    for (int g = 0; g < NG; ++g)
      hv[g] = (16 * g + 4 * q < D) ? *reinterpret_cast<const float4*>(hr + 16 * g) : float4{0.f, 0.f, 0.f, 0.f};
    if (quad) tail.load((size_t)row * C + 4 * q, u);
  };
  float4 hv[NG], hn[NG];
  typename Tail::Regs u{};
  if (wave < ntiles) load_tile(wave, hv, u);
  for (int t = wave; t < ntiles; t += nwaves) {
    const bool more = t + nwaves < ntiles;
    typename Tail::Regs un{};
    if (more) load_tile(t + nwaves, hn, un);
    f32x4 acc = bias;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      acc = mfma16(wf[g].x, hv[g].x, acc);
      acc = mfma16(wf[g].y, hv[g].y, acc);
      acc = mfma16(wf[g].z, hv[g].z, acc);
      acc = mfma16(wf[g].w, hv[g].w, acc);
    }
    const int row = 16 * t + r;
    const int c0 = 4 * q;
    if (row < M && c0 < C) {
      const size_t i0 = (size_t)row * C + c0;
      const float Gl = Tail::NEEDS_G ? G[row % L] : 0.f;
      if ((C & 3) == 0) tail.quad(i0, acc, Gl, u);
      else tail.ragged(i0, min(4, C - c0), acc, Gl);
    }
    if (more) {
#pragma unroll
      for (int g = 0; g < NG; ++g) hv[g] = hn[g];
      u = un;
    }
  }
}

// generic fallback (C > 16): 16 lanes per row, weight in LDS
__global__ void k_unembed(const float* __restrict__ h, const float* __restrict__ Wu, const float* __restrict__ bu,
                          float* __restrict__ score, int M, int C, int D) {
  extern __shared__ float wl[];  // C * D
  for (int i = threadIdx.x; i < C * D; i += blockDim.x) wl[i] = Wu[i];
  __syncthreads();
  constexpr int NI = 8;
  const int sub = threadIdx.x & 15;
  const int rows_per_block = blockDim.x >> 4;
  for (int row = blockIdx.x * rows_per_block + (threadIdx.x >> 4); row < M; row += gridDim.x * rows_per_block) {
    const float* hr = h + (size_t)row * D;
    float hv[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) hv[i] = (sub + 16 * i < D) ? hr[sub + 16 * i] : 0.f;
    for (int c = 0; c < C; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (16 * i < D) acc = fmaf(hv[i], (sub + 16 * i < D) ? wl[c * D + sub + 16 * i] : 0.f, acc);
      acc += __shfl_xor(acc, 8, 16);
      acc += __shfl_xor(acc, 4, 16);
      acc += __shfl_xor(acc, 2, 16);
      acc += __shfl_xor(acc, 1, 16);
      if (sub == 0) score[(size_t)row * C + c] = acc + bu[c];
    }
  }
}

bool unembed_sde_supported(int C, int D) {
  if (C > 16 || D % 4 != 0) return false;
#define X(v) if (D == v) return true;
  FFD_D_LIST(X)
#undef X
  return false;
}

// every tail's launch (requires unembed_sde_supported(C, D))
template <class Tail>
static hipError_t launch_unembed_tail(Tail tail, const float* h, const float* Wu, const float* bu, const float* G, int M,
                                      int L, int C, int D, hipStream_t s) {
  int blocks = cdiv(cdiv(M, 16), 4);
  if (blocks > 2048) blocks = 2048;
  switch (D) {
#define X(d)                                                                                                          \
  case d:                                                                                                             \
    hipLaunchKernelGGL((k_unembed_mfma<d, Tail>), dim3(blocks), dim3(256), 0, s, h, Wu, bu, G, tail, M, L, C); \
    break;
    FFD_D_LIST(X)
#undef X
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_unembed(const float* h, const float* Wu, const float* bu, float* score, int M, int C, int D,
                          hipStream_t s) {
  if (unembed_sde_supported(C, D) && ptr16(h) && ptr16(Wu) && ptr16(score))
    return launch_unembed_tail(TailStore{score}, h, Wu, bu, nullptr, M, 1, C, D, s);
  if (D > 128 || (size_t)C * D * sizeof(float) > 64 * 1024) return hipErrorInvalidValue;
  int blocks = cdiv(M, 16);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_unembed, dim3(blocks), dim3(256), (size_t)C * D * sizeof(float), s, h, Wu, bu, score, M, C, D);
  return hipGetLastError();
}

// x <- SDE step(x, unembed(h)): the fused tail of a sampling step (requires unembed_sde_supported(C, D))
hipError_t launch_unembed_sde(const float* h, const float* Wu, const float* bu, float* x, const float* z, const float* G,
                              SdeParams p, uint64_t seed, uint64_t elem_offset, uint32_t step, int B, int L, int C,
                              int D, hipStream_t s) {
  if (!unembed_sde_supported(C, D) || !ptr16(h) || !ptr16(Wu)) return hipErrorInvalidValue;
  if ((C & 3) == 0 && (!ptr16(x) || !ptr16(z))) return hipErrorInvalidValue;  // x / z quads
  if ((C & 3) == 0 && (elem_offset & 3)) return hipErrorInvalidValue;
  return launch_unembed_tail(TailSde{x, p, Draws{z, seed, elem_offset, step}}, h, Wu, bu, G, B * L, L, C, D, s);
}

// tail(x, unembed(h)): the fused tail of an ODE interval (requires unembed_sde_supported(C, D)); xp / d1 as in
// launch_ode_step (unused by ODE_EULER)
hipError_t launch_unembed_ode(int tail, const float* h, const float* Wu, const float* bu, float* x, float* xp, float* d1,
                              const float* G, SdeParams p, int B, int L, int C, int D, hipStream_t s) {
  if (!unembed_sde_supported(C, D) || !ptr16(h) || !ptr16(Wu)) return hipErrorInvalidValue;
  if ((C & 3) == 0 && (!ptr16(x) || !ptr16(xp) || !ptr16(d1))) return hipErrorInvalidValue;  // quads
  if (tail != ODE_EULER && (!xp || !d1)) return hipErrorInvalidValue;
  switch (tail) {
    case ODE_EULER: return launch_unembed_tail(TailOde<ODE_EULER>{x, nullptr, nullptr, p}, h, Wu, bu, G, B * L, L, C, D, s);
    case ODE_PREDICT: return launch_unembed_tail(TailOde<ODE_PREDICT>{x, xp, d1, p}, h, Wu, bu, G, B * L, L, C, D, s);
    case ODE_CORRECT: return launch_unembed_tail(TailOde<ODE_CORRECT>{x, xp, d1, p}, h, Wu, bu, G, B * L, L, C, D, s);
    default: return hipErrorInvalidValue;
  }
}

// multistep tail(x, hist, unembed(h)): the fused tail of a multistep interval (requires unembed_sde_supported(C, D))
hipError_t launch_unembed_multistep(const float* h, const float* Wu, const float* bu, float* x, float* hist, const float* G,
                                    MultistepParams p, int have_prev, int B, int L, int C, int D, hipStream_t s) {
  if (!unembed_sde_supported(C, D) || !ptr16(h) || !ptr16(Wu) || !hist) return hipErrorInvalidValue;
  if ((C & 3) == 0 && (!ptr16(x) || !ptr16(hist))) return hipErrorInvalidValue;  // quads
  if (have_prev) return launch_unembed_tail(TailMultistep<true>{x, hist, p}, h, Wu, bu, G, B * L, L, C, D, s);
  return launch_unembed_tail(TailMultistep<false>{x, hist, p}, h, Wu, bu, G, B * L, L, C, D, s);
}

// ---------------------------------------------------------------------------
// KV table store: table[h][l][:] <- sample 0's head-major K/V rows, l < n (Q1)
// ---------------------------------------------------------------------------
__global__ void k_kv_store(const float* __restrict__ k, const float* __restrict__ v, float* __restrict__ kt,
                           float* __restrict__ vt, int L, int H, int hd, int n) {
  const int per_head = n * hd;
  const int total = H * per_head;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int h = i / per_head, r = i - h * per_head;
    const size_t off = (size_t)h * L * hd + r;  // sample 0: (0*H + h)*L*hd
    kt[off] = k[off];
    vt[off] = v[off];
  }
}

hipError_t launch_kv_store(const float* k, const float* v, float* kt, float* vt, int L, int H, int hd, int n,
                           hipStream_t s) {
  if (n <= 0) return hipSuccess;
  int blocks = cdiv(n * H * hd, 256);
  hipLaunchKernelGGL(k_kv_store, dim3(blocks), dim3(256), 0, s, k, v, kt, vt, L, H, hd, n);
  return hipGetLastError();
}

// predict_hermite's last step (fourier.py:470-495): prediction = sum_k w_k * history[k]; the K weights come
// from the (order+1)^2 normal equations solved on the host.
struct WeightVec { float w[32]; };
__global__ void k_weighted_sum(const float* __restrict__ hist, WeightVec wv, float* __restrict__ out, int K, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(wv.w[k], hist[(size_t)k * n + i], acc);
    out[i] = acc;
  }
}

static hipError_t launch_weighted_sum(const float* hist, const float* w_host, float* out, int K, size_t n, hipStream_t s) {
  if (K < 1 || K > 32) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  WeightVec wv{};
  for (int k = 0; k < K; ++k) wv.w[k] = w_host[k];
  const int blocks = (int)std::min<size_t>((n + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(k_weighted_sum, dim3(blocks), dim3(256), 0, s, hist, wv, out, K, n);
  return hipGetLastError();
}

SdeParams sde_params(int sde, double a, double b, double t, float step_size) {
  SdeParams p{};
  p.sde = sde;
  if (sde == FFD_SDE_VP) {
    const double beta = a + t * (b - a);  // sde.py:212-213
    p.a = (float)(-0.5 * beta);
    p.cs = (float)sqrt(beta);
  } else {
    const double r = b / a;
    p.cs = (float)(a * sqrt(2.0 * log(r)) * pow(r, t));  // sde.py:143-147
    p.a = 0.f;
  }
  p.dt = step_size;
  p.sqdt = sqrtf(step_size);
  return p;
}

// (log alpha, log sigma) of the forward marginal at t (sde.py:106-123, 186-210; without G).  VP: sigma^2 =
// -expm1(2 log alpha), so that small t loses nothing to 1 - exp(.).
static void log_alpha_sigma(int sde, double a, double b, double t, double* la, double* ls) {
  if (sde == FFD_SDE_VP) {
    *la = -0.25 * t * t * (b - a) - 0.5 * t * a;
    *ls = 0.5 * log(-expm1(2.0 * *la));
  } else {
    *la = 0.0;
    *ls = log(a) + t * log(b / a);
  }
}

int multistep_coef(int sde, double a, double b, int solver, double t_prev, double t, double t_next, double step_size,
                   int have_prev, double* c) {
  if (!c || (sde != FFD_SDE_VP && sde != FFD_SDE_VE)) return FFD_ERR_INVALID;
  if (!(t_next < t) || (have_prev && !(t < t_prev))) return FFD_ERR_INVALID;
  if (solver == FFD_SOLVER_ODE_AB2) {
    if (!(step_size > 0.0)) return FFD_ERR_INVALID;
    double cs;  // f = qa x and g = cs at t, in sde_params' expressions
    if (sde == FFD_SDE_VP) {
      const double beta = a + t * (b - a);
      c[0] = -0.5 * beta, cs = sqrt(beta);
    } else {
      const double r = b / a;
      c[0] = 0.0, cs = a * sqrt(2.0 * log(r)) * pow(r, t);
    }
    c[1] = -0.5 * cs * cs;
    c[2] = 0.0;
    c[3] = have_prev ? -1.5 * step_size : -step_size;
    c[4] = have_prev ? 0.5 * step_size : 0.0;
  } else if (solver == FFD_SOLVER_DPMPP_2M) {
    double la, ls, lan, lsn;
    log_alpha_sigma(sde, a, b, t, &la, &ls);
    log_alpha_sigma(sde, a, b, t_next, &lan, &lsn);
    if (!std::isfinite(ls) || !std::isfinite(lsn)) return FFD_ERR_INVALID;  // sigma == 0
    const double h = (lan - lsn) - (la - ls);
    const double cc = -exp(lan) * expm1(-h);
    c[0] = exp(-la);
    c[1] = exp(2.0 * ls - la);
    c[2] = expm1(lsn - ls);
    c[3] = cc, c[4] = 0.0;
    if (have_prev) {
      double lap, lsp;
      log_alpha_sigma(sde, a, b, t_prev, &lap, &lsp);
      if (!std::isfinite(lsp)) return FFD_ERR_INVALID;
      const double r = ((la - ls) - (lap - lsp)) / h;
      c[3] = cc * (1.0 + 1.0 / (2.0 * r));
      c[4] = -cc / (2.0 * r);
    }
  } else {
    return FFD_ERR_INVALID;
  }
  for (int i = 0; i < 5; ++i)
    if (!std::isfinite(c[i])) return FFD_ERR_INVALID;
  return FFD_OK;
}

MultistepParams multistep_params(const double* c) {
  return MultistepParams{(float)c[0], (float)c[1], (float)c[2], (float)c[3], (float)c[4]};
}

// (a, sg) of the forward transition s -> t in double (include/ffd.h ffd_host_transition_coef).  One operation per
// statement: the float64 restatement of the tests repeats them in this order.
int transition_coef(int sde, double a, double b, double s, double t, double* c) {
  if (!c || !std::isfinite(s) || !std::isfinite(t) || s < 0.0 || t < s) return FFD_ERR_INVALID;
  if (sde != FFD_SDE_VP && sde != FFD_SDE_VE) return FFD_ERR_UNSUPPORTED;
  c[0] = 1.0, c[1] = 0.0;
  if (s == t) return FFD_OK;
  if (sde == FFD_SDE_VP) {
    const double lt = -0.25 * t * t * (b - a) - 0.5 * t * a;
    const double ls = -0.25 * s * s * (b - a) - 0.5 * s * a;
    const double d = lt - ls;
    c[0] = exp(d);
    c[1] = sqrt(-expm1(2.0 * d));
  } else {
    const double st = a * pow(b / a, t);
    const double ss = a * pow(b / a, s);
    const double vt = st * st;
    const double vs = ss * ss;
    const double v = vt - vs;
    c[1] = sqrt(v > 0.0 ? v : 0.0);
  }
  return FFD_OK;
}

}  // namespace ffd

// ---- C ABI (include/ffd.h): the context-free entry points on these kernels ----
using namespace ffd;

extern "C" {

int ffd_sde_step(const ffd_sde_desc* sde, float* x, const float* score, const float* G, double t, float step_size,
                 const float* z, uint64_t seed, uint64_t sample_offset, int step, int B, int L, int C, void* stream) {
  if (!sde || !x || !score || !G || B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  if (sde->sde != FFD_SDE_VP && sde->sde != FFD_SDE_VE) return FFD_ERR_UNSUPPORTED;
  if (!(step_size > 0.f)) return FFD_ERR_INVALID;  // sde.py:157,238 assert
  hipError_t e = launch_sde_step(x, score, z, G, sde_params(sde->sde, sde->a, sde->b, t, step_size), seed,
                                 sample_offset * (uint64_t)L * C, (uint32_t)step, B, L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_host_transition_coef(const ffd_sde_desc* sde, double s, double t, double coef_out[2]) {
  if (!sde) return FFD_ERR_INVALID;
  return transition_coef(sde->sde, sde->a, sde->b, s, t, coef_out);
}

int ffd_forward_transition(const ffd_sde_desc* sde, float* x, const float* G, double s, double t, const float* z,
                           uint64_t seed, uint64_t sample_offset, uint32_t tag, int B, int L, int C, void* stream) {
  if (!sde || !x || !G || B < 1 || L < 1 || C < 1 || x == z) return FFD_ERR_INVALID;
  double c[2];
  if (int rc = transition_coef(sde->sde, sde->a, sde->b, s, t, c)) return rc;
  hipError_t e = launch_forward_transition(x, G, (float)c[0], (float)c[1], z, seed, sample_offset * (uint64_t)L * C, tag, B,
                                           L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

// the argument checks the three ODE operators share (before any device work)
static int ode_args(const ffd_sde_desc* sde, const void* x, const void* score, const void* G, float step_size, int B, int L,
                    int C) {
  if (!sde || !x || !score || !G || B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  if (!(step_size > 0.f)) return FFD_ERR_INVALID;
  if (sde->sde != FFD_SDE_VP && sde->sde != FFD_SDE_VE) return FFD_ERR_UNSUPPORTED;
  return FFD_OK;
}

int ffd_ode_step(const ffd_sde_desc* sde, float* x, const float* score, const float* G, double t, float step_size, int B,
                 int L, int C, void* stream) {
  if (int rc = ode_args(sde, x, score, G, step_size, B, L, C)) return rc;
  hipError_t e = launch_ode_step(ODE_EULER, x, score, nullptr, nullptr, G, sde_params(sde->sde, sde->a, sde->b, t, step_size),
                                 B, L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_ode_heun_predict(const ffd_sde_desc* sde, const float* x, const float* score, const float* G, double t,
                         float step_size, float* x_pred_out, float* drift_out, int B, int L, int C, void* stream) {
  if (int rc = ode_args(sde, x, score, G, step_size, B, L, C)) return rc;
  if (!x_pred_out || !drift_out || x_pred_out == x || drift_out == x || x_pred_out == drift_out) return FFD_ERR_INVALID;
  hipError_t e = launch_ode_step(ODE_PREDICT, const_cast<float*>(x), score, x_pred_out, drift_out, G,
                                 sde_params(sde->sde, sde->a, sde->b, t, step_size), B, L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_ode_heun_correct(const ffd_sde_desc* sde, float* x, const float* x_pred, const float* score_pred, const float* drift,
                         const float* G, double t_next, float step_size, int B, int L, int C, void* stream) {
  if (int rc = ode_args(sde, x, score_pred, G, step_size, B, L, C)) return rc;
  if (!x_pred || !drift || x_pred == x || drift == x) return FFD_ERR_INVALID;
  hipError_t e = launch_ode_step(ODE_CORRECT, x, score_pred, const_cast<float*>(x_pred), const_cast<float*>(drift), G,
                                 sde_params(sde->sde, sde->a, sde->b, t_next, step_size), B, L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_host_multistep_coef(const ffd_sde_desc* sde, int solver, double t_prev, double t, double t_next, double step_size,
                            int have_prev, double* coef_out) {
  if (!sde || !coef_out) return FFD_ERR_INVALID;
  double c[5];  // coef_out is written on success only
  if (int rc = multistep_coef(sde->sde, sde->a, sde->b, solver, t_prev, t, t_next, step_size, have_prev, c)) return rc;
  for (int i = 0; i < 5; ++i) coef_out[i] = c[i];
  return FFD_OK;
}

int ffd_ode_multistep_step(float* x, const float* score, const float* G, float* hist, const double* coef, int have_prev,
                           int B, int L, int C, void* stream) {
  if (!x || !score || !G || !hist || !coef || B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  if (hist == x || hist == score) return FFD_ERR_INVALID;
  const MultistepParams p = multistep_params(coef);
  for (float v : {p.qa, p.qb, p.cxm1, p.cn, p.cp})
    if (!std::isfinite(v)) return FFD_ERR_INVALID;
  if (!have_prev && coef[4] != 0.0) return FFD_ERR_INVALID;
  hipError_t e = launch_multistep_step(x, score, hist, G, p, have_prev, B, L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_prior(const ffd_sde_desc* sde, float* x, const float* z, const float* G, uint64_t seed, uint64_t sample_offset,
              int B, int L, int C, void* stream) {
  if (!sde || !x || !G || B < 1 || L < 1 || C < 1) return FFD_ERR_INVALID;
  const float scale = (sde->sde == FFD_SDE_VE) ? (float)sde->b : 1.0f;
  hipError_t e = launch_prior(x, z, G, scale, seed, sample_offset * (uint64_t)L * C, B, L, C, (hipStream_t)stream);
  return e == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_positional_encoding(const float* x, float* weight, float* out, int B, int L, int D, float max_norm,
                            void* stream) {
  if (!x || !weight || !out || B < 1 || L < 1 || D < 1) return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  // nn.Embedding(max_norm) renormalises the looked-up rows in place at every forward (transformer.py:13-15,26)
  if (max_norm > 0.f && launch_renorm_rows_once(weight, L, D, max_norm, s) != hipSuccess) return FFD_ERR_HIP;
  return launch_add_table(x, weight, nullptr, out, B, L, D, s) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

int ffd_time_encoding(const float* x, const float* timesteps, const float* W, const float* dense_w,
                      const float* dense_b, float* temb_work, float* out, int B, int L, int D, void* stream) {
  if (!x || !timesteps || !W || !dense_w || !dense_b || !temb_work || !out || B < 1 || L < 1 || D < 1)
    return FFD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (launch_time_embed(timesteps, 0.f, B, W, dense_w, dense_b, temb_work, D, s) != hipSuccess) return FFD_ERR_HIP;
  return launch_add_table(x, nullptr, temb_work, out, B, L, D, s) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

// Hermite polynomials H_0..H_order at s (fourier.py:341-394: physicists' recurrence)
static void hermite_row(double s, int order, double* H) {
  H[0] = 1.0;
  if (order >= 1) H[1] = 2.0 * s;
  for (int n = 1; n < order; ++n) H[n + 1] = 2.0 * s * H[n] - 2.0 * n * H[n - 1];
}

int ffd_hermite_predict(const float* history, const double* timesteps, double target, int order, float* out, int K,
                        size_t n, void* stream) {
  if (!history || !timesteps || !out || K < 1 || K > 32 || order < 0 || order > 8) return FFD_ERR_INVALID;
  float w[32] = {0};
  double tmin = timesteps[0], tmax = timesteps[0];
  for (int k = 1; k < K; ++k) tmin = std::min(tmin, timesteps[k]), tmax = std::max(tmax, timesteps[k]);
  if (K < 2 || tmax == tmin) {
    w[K - 1] = 1.f;  // fourier.py:416-428: not enough history -> last value
  } else {
    const int P = order + 1;
    auto norm = [&](double t) {  // fourier.py:431-441, values held in fp32 tensors and clamped to [-1,1]
      double v = (double)(float)(2.0 * (t - tmin) / (tmax - tmin) - 1.0);
      return std::min(1.0, std::max(-1.0, v));
    };
    double Hm[32][9], Ht[9], A[9][18];
    for (int k = 0; k < K; ++k) hermite_row(norm(timesteps[k]), order, Hm[k]);
    hermite_row(norm(target), order, Ht);
    // normal equations with ridge 1e-6 (fourier.py:462-466), inverted by Gauss-Jordan with partial pivoting
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < P; ++j) {
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc += Hm[k][i] * Hm[k][j];
        A[i][j] = acc + (i == j ? 1e-6 : 0.0);
        A[i][P + j] = i == j ? 1.0 : 0.0;
      }
    for (int c = 0; c < P; ++c) {
      int piv = c;
      for (int r = c + 1; r < P; ++r)
        if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
      if (A[piv][c] == 0.0) return FFD_ERR_INVALID;
      if (piv != c)
        for (int j = 0; j < 2 * P; ++j) std::swap(A[c][j], A[piv][j]);
      const double inv = 1.0 / A[c][c];
      for (int j = 0; j < 2 * P; ++j) A[c][j] *= inv;
      for (int r = 0; r < P; ++r)
        if (r != c) {
          const double f = A[r][c];
          if (f != 0.0)
            for (int j = 0; j < 2 * P; ++j) A[r][j] -= f * A[c][j];
        }
    }
    // w_k = H_target . (HtH)^-1 . H_k   (prediction = sum_k w_k history_k, fourier.py:476-481)
    for (int k = 0; k < K; ++k) {
      double acc = 0.0;
      for (int i = 0; i < P; ++i) {
        double u = 0.0;
        for (int j = 0; j < P; ++j) u += A[i][P + j] * Hm[k][j];
        acc += Ht[i] * u;
      }
      w[k] = (float)acc;
    }
  }
  return launch_weighted_sum(history, w, out, K, n, (hipStream_t)stream) == hipSuccess ? FFD_OK : FFD_ERR_HIP;
}

}  // extern "C"
