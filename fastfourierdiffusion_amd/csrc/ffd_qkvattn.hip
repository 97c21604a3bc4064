// Fused in-projection + attention: one workgroup per (sample, head).
//
// Why: with separate kernels the (B,H,L,hd) q/k/v tensors make a round trip through HBM every layer
// (83 MB written + 83 MB read at B=512 ECG): the projection kernel's copy-out alone is write-bandwidth
// bound (21 of its 57 us) and the attention kernel spends ~28 us staging them back.  Here the head's
// q, k, v rows are produced by the matrix cores straight into the LDS images the attention phase reads
// (Q^T [dim][token], K^T [dim][token], V [token][8]) and never exist in global memory.
//
// Phase 1 (projection, v_mfma_f32_16x16x4_f32): D[token][feature] = x[token][:] . W_h[feature][:] for the
// head's 3*hd features (q | k | v rows of in_proj, score_models.py:61-66 -> nn.MultiheadAttention), in one or
// two 16-feature tiles.  x rows go from global memory directly into the A operand -- each lane holds 4
// consecutive k of its token per 16-wide chunk (float4), the weight pack uses the same k permutation --
// and the softmax scale log2(e)/sqrt(hd) is folded into the q rows of the pack.
// Phase 2 (attention, attend_qtiles: one routine for both kernels): S^T tiles on v_mfma_f32_32x32x2_f32 with the
// stale-max reference riding on contraction dim hd (skipped while it is zero), packed-fp32 softmax / P.V, V rows
// pipelined from LDS.
//
// E2-CRF cache modes (cached_transformer.py:237-305): `n_own` leading tokens take K/V from the projection,
// the rest from the shared tables (kt/vt != NULL); PURE (n_own = 0) runs with the q-only weight pack; in
// MIXED the workgroups of batch element 0 also write their recomputed rows back to the tables
// (caching.py:326-328).
#include <type_traits>

#include "ffd_internal.h"

namespace ffd {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// acc += p.lo * v  /  acc += p.hi * v  with the scalar broadcast done by the instruction's operand select (no v_mov to
// build a {p, p} pair: 16 of the ~93 vector instructions of a 32x32 score tile): p is a pair of adjacent accumulator
// registers of the S^T tile.  The same FMAs, bit for bit.
__device__ __forceinline__ f32x2 pk_fma_lo(f32x2 p, f32x2 v, f32x2 acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(p), "v"(v));
  return acc;
}
__device__ __forceinline__ f32x2 pk_fma_hi(f32x2 p, f32x2 v, f32x2 acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(p), "v"(v));
  return acc;
}

// Diagnostics (STAMP instances only; ffd_probe_attn): per-wave record of 16 x u64 in a buffer nothing else reads --
// [0] 100 MHz real time at entry, shader-clock stamps [1] entry, [2] projection begin (x requested, weights staged),
// [3] projection end, [4] attention begin (tables / norms done), [5] attention end, [6] exit, then shader cycles summed
// over the wave's key tiles: [7] K fragments + QK^T until the scores are readable, [8] mask + softmax, [9] P.V;
// [10] key tiles walked, [11] hardware id (HW_ID), [12] 100 MHz real time at exit.
#define FFD_STAMP_T() ((unsigned long long)__builtin_amdgcn_s_memtime())
struct WaveStamps {
  unsigned long long t[7] = {0, 0, 0, 0, 0, 0, 0}, qk = 0, sm = 0, pv = 0, n = 0;  // [0 .. 6], [7], [8], [9], [10]
  __device__ __forceinline__ void begin() { t[0] = __builtin_amdgcn_s_memrealtime(), t[1] = FFD_STAMP_T(); }
  // lane 0 of each wave writes record (workgroup, wave) at kernel exit
  __device__ __forceinline__ void write(unsigned long long* stamp, int nwaves) {
    if ((threadIdx.x & 63) == 0 && stamp != nullptr) {
      unsigned long long* r = stamp + ((size_t)blockIdx.x * nwaves + (threadIdx.x >> 6)) * 16;
      t[6] = FFD_STAMP_T();
#pragma unroll
      for (int i = 0; i < 7; ++i) r[i] = t[i];
      r[7] = qk, r[8] = sm, r[9] = pv, r[10] = n, r[11] = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));
      r[12] = __builtin_amdgcn_s_memrealtime();
    }
  }
};

// ---- weight pack ---------------------------------------------------------------------------------
// awp[h][ct][step4][lane][4]: the B operand of k-step (4*step4 + i) for lane (n = lane & 15, q = lane >> 4):
//   full 16-chunks j < D/16 : k = 16 j + 4 q + i          (step4 = j)
//   remainder (D % 16) / 4 steps : k = 16 (D/16) + 4 i + q   (step4 = D/16, i < rem steps)
// feature fi = 16 ct + n -> (reg, e) = (fi / hd, fi % hd) for fi < nf (= 3 hd, or hd for the q-only pack).
__global__ void k_pack_attn(const float* __restrict__ W, const float* __restrict__ b, float* __restrict__ awp,
                            float* __restrict__ abp, int D, int H, int hd, int hpw, int nct, int q_only, float qscale) {
  // one pack per head group (hpw consecutive heads): feature fi -> head hh = fi / fph, then (reg, e)
  const int steps4 = (D + 15) / 16;
  const int NG = H / hpw;
  // q_only is the pack MODE: 0 q | k | v of every head in feature order, 1 q only, 2 (one head per group) tile 0 = k | v,
  // tile 1 = q -- the split small-batch form projects tile 1 for its own q-tiles' tokens only
  const bool kvq = q_only == 2;
  const int fph = q_only == 1 ? hd : 3 * hd;  // features per head
  const int nf = kvq ? 32 : hpw * fph;
  const int total = NG * nct * steps4 * 64 * 4;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int i = idx & 3, lane = (idx >> 2) & 63;
    int rest = idx >> 8;
    const int j = rest % steps4;
    rest /= steps4;
    const int ct = rest % nct, hg = rest / nct;
    const int n = lane & 15, q = lane >> 4;
    const int fi = 16 * ct + n;
    int k;
    if (16 * j + 16 <= D) k = 16 * j + 4 * q + i;
    else k = (4 * i < D - 16 * j) ? 16 * j + 4 * i + q : -1;
    float v = 0.f;
    if (fi < nf && k >= 0 && k < D) {
      int hh = fi / fph, f = fi - hh * fph;
      int reg = f / hd, e = f - reg * hd;
      bool on = true;
      if (kvq) {  // tile 0: k[0 .. hd), v[0 .. hd); tile 1: q[0 .. hd)
        hh = 0, on = n < (ct == 0 ? 2 * hd : hd) && ct < 2;
        reg = ct == 0 ? (n < hd ? 1 : 2) : 0, e = ct == 0 ? (n < hd ? n : n - hd) : n;
      }
      if (on) v = W[(size_t)(reg * D + (hg * hpw + hh) * hd + e) * D + k] * (reg == 0 ? qscale : 1.f);
    }
    awp[idx] = v;
  }
  const int nb = NG * nct * 16;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nb; idx += gridDim.x * blockDim.x) {
    const int n = idx & 15, ct = (idx >> 4) % nct, hg = (idx >> 4) / nct;
    const int fi = 16 * ct + n;
    float v = 0.f;
    if (fi < nf) {
      int hh = fi / fph, f = fi - hh * fph;
      int reg = f / hd, e = f - reg * hd;
      bool on = true;
      if (kvq) {
        hh = 0, on = n < (ct == 0 ? 2 * hd : hd) && ct < 2;
        reg = ct == 0 ? (n < hd ? 1 : 2) : 0, e = ct == 0 ? (n < hd ? n : n - hd) : n;
      }
      if (on) v = b[reg * D + (hg * hpw + hh) * hd + e] * (reg == 0 ? qscale : 1.f);
    }
    abp[idx] = v;
  }
}

static int attn_nct(int hd, int hpw, int q_only) { return q_only == 2 ? 2 : cdiv(hpw * (q_only ? hd : 3 * hd), 16); }
// head dims for which the kv | q pack exists: a head's k and v fit one 16-wide tile and q | k | v need two anyway
bool attn_kvq_supported(int hd) { return 2 * hd <= 16 && 3 * hd > 16; }

size_t attn_pack_floats(int D, int H, int hpw, int q_only) {
  const int nct = attn_nct(D / H, hpw, q_only);
  return (size_t)(H / hpw) * nct * ((D + 15) / 16) * 256 + (size_t)(H / hpw) * nct * 16;
}

float attn_q_scale(int hd) { return 1.4426950408889634f / sqrtf((float)hd); }

hipError_t launch_pack_attn(const float* in_w, const float* in_b, float* pack, int D, int H, int hpw, int q_only,
                            hipStream_t s) {
  const int hd = D / H;
  const int nct = attn_nct(hd, hpw, q_only);
  float* abp = pack + (size_t)(H / hpw) * nct * ((D + 15) / 16) * 256;
  const float qscale = attn_q_scale(hd);
  hipLaunchKernelGGL(k_pack_attn, dim3(64), dim3(256), 0, s, in_w, in_b, pack, abp, D, H, hd, hpw, nct, q_only, qscale);
  return hipGetLastError();
}

// max over the wave of a non-negative value: four DPP steps inside each row of 16 lanes, two xor-shuffles across the rows
__device__ __forceinline__ float wave_max_nonneg(float v) {
#define FFD_DPP_MAX(ctrl) \
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, true)))
  FFD_DPP_MAX(0xB1);   // quad_perm [1, 0, 3, 2]
  FFD_DPP_MAX(0x4E);   // quad_perm [2, 3, 0, 1]
  FFD_DPP_MAX(0x141);  // row_half_mirror
  FFD_DPP_MAX(0x140);  // row_mirror
#undef FFD_DPP_MAX
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}

// Largest squared norm of the head's (scaled) q rows and of its k rows: nrm[0] keys, nrm[1] queries (as the bit patterns
// of non-negative floats, which order like unsigned integers: reduced inside the wave, then ONE LDS atomic max per wave
// and value -- an atomic per lane serialises on the one address: 24 k cycles of the L = 512 kernel's 140 k when tried).
// |q . k| <= |q| |k| bounds every score of the head; while that bound is within the threshold T the online softmax
// needs no running maximum (its reference stays 0) and the key-tile loop skips the max reduction, the cross-half
// exchange and the refresh test.  The caller zeroes nrm[0..1] before the barrier that precedes this call.
template <int HD>
__device__ __forceinline__ void head_norms(const float* kts, const float* qts, unsigned* nrm, int Lp, int LS, int tid, int nthreads,
                                           int jq0 = 0, int jq1 = 1 << 30) {  // q rows [jq0, jq1) only
  float km = 0.f, qm = 0.f;
  for (int j = tid; j < Lp; j += nthreads) {
    float k2 = 0.f, q2 = 0.f;
    const bool qon = j >= jq0 && j < jq1;
#pragma unroll
    for (int e = 0; e < HD; ++e) {
      const float kv = kts[e * LS + j], qv = qon ? qts[e * LS + j] : 0.f;
      k2 = fmaf(kv, kv, k2), q2 = fmaf(qv, qv, q2);
    }
    km = fmaxf(km, k2), qm = fmaxf(qm, q2);
  }
  km = wave_max_nonneg(km), qm = wave_max_nonneg(qm);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(nrm, __float_as_uint(km));
    atomicMax(nrm + 1, __float_as_uint(qm));
  }
}

// One head's LDS images at row stride LS: V [Lp][8] | K^T [2 KST][LS] | Q^T [2 KST][LS] (Q^T already scaled by
// log2(e)/sqrt(hd)).  Dims e of the 32x32x2 QK^T sit in k-pair step e / 2, half e % 2; one more step carries -m_ref.
template <int HD>
struct HeadDims {
  static constexpr int KST = (HD + 1) / 2;  // k-steps of the head dims
  static constexpr int KSX = (HD + 2) / 2;  // ... with the -m_ref step
  static constexpr int SX = HD / 2;         // the -m_ref step's index
  static constexpr int HX = HD & 1;         // ... and the half that carries it
  static constexpr int HP = (HD + 1) / 2;   // output feature pairs per row
  static constexpr float T = ATTN_SCORE_T;  // scores (log2 domain) may sit this far from the reference before it is refreshed
  static constexpr size_t floats(int LS) { return (size_t)LS * (8 + 4 * KST); }  // V | K^T | Q^T
};

// every score of the head is within +- sqrt(max |q|^2 max |k|^2) (wave-uniform; after the barrier behind head_norms)
template <int HD>
__device__ __forceinline__ bool head_bounded(const unsigned* nrm) {
  constexpr float T = HeadDims<HD>::T;
  return __builtin_amdgcn_ballot_w64(__uint_as_float(nrm[1]) * __uint_as_float(nrm[0]) <= T * T) != 0;
}

// XCD-aware mapping of workgroup `pair` to (sample b, head or head group g of NG): workgroups are dealt round-robin to the
// 8 XCDs (blockIdx % 8), each with its own L2.  All groups of a sample read the same x rows, so they are placed on one
// XCD: x is fetched into one L2 once instead of into (up to) eight.
__device__ __forceinline__ void xcd_sample_group(int pair, int B, int NG, int& b, int& g) {
  const int nmain = (B >> 3) * 8 * NG;
  if (pair < nmain) {
    const int xcd = pair & 7, slot = pair >> 3;
    const int sb = slot / NG;
    b = sb * 8 + xcd, g = slot - sb * NG;
  } else {
    b = pair / NG, g = pair - b * NG;
  }
}

// Rows served by the shared tables (PURE: all of them; MIXED: tokens >= n_own) overwrite / fill head h's K^T and V,
// by threads tid of nthreads.  (I is the caller's index type: the compiler unrolls a loop over unsigned threadIdx /
// blockDim strides differently from one over int strides, so each kernel keeps the loops it had.)
template <int HD, typename I>
__device__ __forceinline__ void fill_from_tables(float* vs, float* kts, int LS, const float* kt, const float* vt, int h,
                                                 int L, int Lp, int n_own, int q_only, I tid, I nthreads) {
  if (!q_only && n_own > 0) __syncthreads();  // MIXED: the projection wrote these rows first
  const float* ktab = kt + (size_t)h * L * HD;
  const float* vtab = vt + (size_t)h * L * HD;
  for (int j = n_own + tid; j < L; j += nthreads) {
    float kx[HD], vx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) vx[e] = 0.f;
    const float* kp = ktab + (size_t)j * HD;
    const float* vp = vtab + (size_t)j * HD;
    if constexpr (HD % 2 == 0) {
#pragma unroll
      for (int e = 0; e < HD; e += 2) {
        const float2 a = *reinterpret_cast<const float2*>(kp + e);
        const float2 c2 = *reinterpret_cast<const float2*>(vp + e);
        kx[e] = a.x, kx[e + 1] = a.y, vx[e] = c2.x, vx[e + 1] = c2.y;
      }
    } else {
#pragma unroll
      for (int e = 0; e < HD; ++e) kx[e] = kp[e], vx[e] = vp[e];
    }
#pragma unroll
    for (int e = 0; e < HD; ++e) kts[e * LS + j] = kx[e];
    *reinterpret_cast<float4*>(vs + (size_t)j * 8) = float4{vx[0], vx[1], vx[2], vx[3]};
    *reinterpret_cast<float4*>(vs + (size_t)j * 8 + 4) = float4{vx[4], vx[5], vx[6], vx[7]};
  }
  if (q_only) {  // PURE: key rows in [L, Lp) were never written; they are masked but must be finite
    for (int j = L + tid; j < Lp; j += nthreads) {
#pragma unroll
      for (int e = 0; e < HD; ++e) kts[e * LS + j] = 0.f;
      *reinterpret_cast<float4*>(vs + (size_t)j * 8) = float4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<float4*>(vs + (size_t)j * 8 + 4) = float4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// MIXED: batch element 0 publishes head h's recomputed rows (tokens < n_own; caching.py:326-328,
// cached_transformer.py:301-305), by threads tid of nthreads (I: see fill_from_tables)
template <int HD, typename I>
__device__ __forceinline__ void publish_kv(const float* vs, const float* kts, int LS, float* kt_out, float* vt_out, int h,
                                           int L, int n_own, I tid, I nthreads) {
  for (int idx = tid; idx < n_own * HD; idx += nthreads) {
    const int j = idx / HD, e = idx - j * HD;
    kt_out[(size_t)h * L * HD + idx] = kts[e * LS + j];
    vt_out[(size_t)h * L * HD + idx] = vs[(size_t)j * 8 + e];
  }
}

// per query row of a wave's QG q-tiles: reference exponent, row sum and unnormalised output (pairs of the two halves)
template <int HD, int QG>
struct QRows {
  float mref[QG];
  f32x2 lsum[QG], acc[QG][HeadDims<HD>::HP];
};

// The images as LDS pointers: the compiler optimises the routine before inlining it, and with generic pointers it
// plans the LDS addressing as if they could point anywhere (more registers in most instances).
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) const float lds_f32;
typedef __attribute__((address_space(3))) const float4 lds_f32x4;
#else  // (the host pass parses the routine too)
typedef const float lds_f32;
typedef const float4 lds_f32x4;
#endif

// ---- phase 1's store plan ----------------------------------------------------------------------------
// Where a lane's feature of a 16-token projection tile goes.  The lane holds the feature for four consecutive tokens;
// in a Q^T / K^T row they are 4 bytes apart, in the V image ([token][8]) 32.  Both shapes are four ds_write_b32 at
// a, a + s, a + 2 s, a + 3 s with per-lane a and s; left to the compiler, it re-derives a and the three offsets with
// selects on the lane's kind in every tile (~ 9 vector instructions per feature tile).  Here the byte address of the
// wave's first tile, the three offsets and the step to the wave's next tile are worked out once in front of the tile
// loop and made opaque (the empty asm), so that a tile costs three adds for the addresses and one for the step.
// Same values to the same addresses in the same order.  (k_qkv_attention_mh only: in k_qkv_attention the five registers
// per feature tile cost its 128-register instances scratch and two others a wave of occupancy.)
struct StorePlan {
  unsigned a, s1, s2, s3, step;
  // image_float: float index of the feature's token 0 in LDS (V row: of its column); tok: first token of the lane's four
  // in the wave's first tile; tile_tokens: tokens between two tiles of the wave
  __device__ __forceinline__ void init(const float* lds0, int image_float, bool vrow, int tok, int tile_tokens) {
    unsigned s = vrow ? 32u : 4u;
    asm("" : "+v"(s));  // (one select; the rest is arithmetic on it)
    a = lds_addr(lds0) + 4u * (unsigned)image_float + (unsigned)tok * s;
    s1 = s, s2 = s + s, s3 = s2 + s, step = (unsigned)tile_tokens * s;
    asm("" : "+v"(a), "+v"(s1), "+v"(s2), "+v"(s3), "+v"(step));
  }
  __device__ __forceinline__ void store(float x, float y, float z, float w) const {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) float lds_w32;
    *(lds_w32*)(a) = x, *(lds_w32*)(a + s1) = y, *(lds_w32*)(a + s2) = z, *(lds_w32*)(a + s3) = w;
#endif
  }
  __device__ __forceinline__ void next_tile() { a += step; }
};

// ---- phase 2: attention ------------------------------------------------------------------------------
// One wave attends q-tiles qt0 = q_first, q_first + q_step, ... < q_end, QG at a time, over key tiles [t_lo, t_hi) of
// the head's LDS images.  Their row stride is LSC where the kernel has a compile-time one (0: the run-time LSR), so
// that the LDS addresses are per-lane bases + immediate offsets.  STORE: normalise and write query row q to
// orow0 + q * ostride; otherwise (the split form's key pieces) the last q-group's rows are returned unnormalised for
// the caller to merge.  BOUNDED: the head's scores are known to be within T (the layer's static bound), so the reference
// stays 0 for good and its refresh, the -m_ref k-step and their state compile out; the arithmetic that remains is the
// head_bounded = true path's, instruction for instruction.
template <int HD, int QG, bool STAMP, bool STORE, int LSC, bool BOUNDED = false>
__device__ __forceinline__ QRows<HD, QG> attend_qtiles(lds_f32* vs, lds_f32* kts, lds_f32* qts, int LSR,
                                                       int q_first, int q_step, int q_end, int t_lo, int t_hi,
                                                       bool head_bounded, int L, float* orow0, int ostride,
                                                       WaveStamps& st) {
  constexpr int KST = HeadDims<HD>::KST, KSX = HeadDims<HD>::KSX, SX = HeadDims<HD>::SX, HX = HeadDims<HD>::HX;
  constexpr int HP = HeadDims<HD>::HP;
  constexpr float T = HeadDims<HD>::T;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int QT = (L + 31) >> 5;
  const int LS = LSC ? LSC : LSR;
  const bool xlane = half == HX;
  constexpr int PF = 4;
  auto load_v = [&](int r, int kbase, f32x2(&dst)[4]) {
    lds_f32* vr = vs + (size_t)(kbase + (r & 3) + 8 * (r >> 2)) * 8;
    const float4 v0 = *reinterpret_cast<lds_f32x4*>(vr);
    dst[0] = f32x2{v0.x, v0.y}, dst[1] = f32x2{v0.z, v0.w};
    if (HD > 4) {
      const float4 v1 = *reinterpret_cast<lds_f32x4*>(vr + 4);
      dst[2] = f32x2{v1.x, v1.y}, dst[3] = f32x2{v1.z, v1.w};
    } else {
      dst[2] = f32x2{0.f, 0.f}, dst[3] = f32x2{0.f, 0.f};
    }
  };
  QRows<HD, QG> rows;
  for (int qt0 = q_first; qt0 < q_end; qt0 += q_step) {
    float qf[QG][KSX], mref[QG];
    f32x2 lsum[QG], acc[QG][HP];
    bool ref_on = false;  // wave-uniform: some lane of this wave carries a non-zero reference
    bool acc_empty[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) acc_empty[g] = true;
#pragma unroll
    for (int g = 0; g < QG; ++g) {
      const int qtile = (qt0 + g < QT) ? qt0 + g : QT - 1;
#pragma unroll
      for (int s = 0; s < KSX; ++s) {
        const int e = 2 * s + half;
        qf[g][s] = (e < HD) ? qts[e * LS + 32 * qtile + l31] : 0.f;  // dim HD starts at -m_ref = 0
      }
      mref[g] = 0.f;
      lsum[g] = f32x2{0.f, 0.f};
#pragma unroll
      for (int e = 0; e < HP; ++e) acc[g][e] = f32x2{0.f, 0.f};
    }
#pragma unroll 1
    for (int t = t_lo; t < t_hi; ++t) {
      unsigned long long st_a = 0;
      if constexpr (STAMP) st_a = FFD_STAMP_T();
      float kf[KSX];
#pragma unroll
      for (int s = 0; s < KSX; ++s) {
        const int e = 2 * s + half;
        kf[s] = (s < KST && (2 * s + 1 < HD || half == 0)) ? kts[e * LS + 32 * t + l31] : 0.f;
      }
      if (xlane) kf[SX] = 1.0f;
      f32x16 sc[QG];
#pragma unroll
      for (int g = 0; g < QG; ++g) {
        f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < KSX; ++s) {
          if (HD % 2 == 0 && s == SX && !ref_on) continue;  // even hd: that step carries nothing but -m_ref = 0
          z = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[s], qf[g][s], z, 0, 0, 0);
        }
        sc[g] = z;
      }
      const int kbase = 32 * t + 4 * half;
      f32x2 vb[PF][4];
#pragma unroll
      for (int r = 0; r < PF; ++r) load_v(r, kbase, vb[r]);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (STAMP) {  // the stamp follows an instruction that reads the last score tile: QK^T has retired
        asm volatile("v_mov_b32 %0, %0" : "+v"(sc[QG - 1][15]));
        const unsigned long long n = FFD_STAMP_T();
        st.qk += n - st_a, st_a = n, ++st.n;
        __builtin_amdgcn_sched_barrier(0);
      }
      if (32 * t + 32 > L) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          if (32 * t + 8 * r4 + 8 > L) {  // (uniform) registers 4 r4 .. 4 r4 + 3 hold key rows 8 r4 .. 8 r4 + 7 of the tile
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const bool dead = kbase + rr + 8 * r4 >= L;
#pragma unroll
              for (int g = 0; g < QG; ++g) sc[g][4 * r4 + rr] = dead ? -INFINITY : sc[g][4 * r4 + rr];
            }
          }
        }
      }
#pragma unroll
      for (int g = 0; g < QG; ++g) {
        // while the head's bound stays within T and no lane of the wave uses a reference, nothing below can trigger
        if (!BOUNDED && (ref_on || !head_bounded)) {
        float bm = __builtin_fmaxf(__builtin_fmaxf(sc[g][0], sc[g][1]), sc[g][2]);
#pragma unroll
        for (int r = 3; r < 15; r += 2) bm = __builtin_fmaxf(__builtin_fmaxf(bm, sc[g][r]), sc[g][r + 1]);
        bm = __builtin_fmaxf(bm, sc[g][15]);
        const float bmx = fmaxf(bm, __shfl_xor(bm, 32));
        // m_ref starts at 0 and usually stays there: |scores| <= 64 (log2 domain) neither overflow nor lose the row
        // to underflow, and the factor 2^-m_ref cancels in the normalisation whatever it is.
        const bool first = acc_empty[g];  // nothing accumulated yet: this is the row's first key tile
        const bool refresh = first ? (fabsf(bmx) > T) : (bmx > T);
        if (__builtin_amdgcn_ballot_w64(refresh) != 0) ref_on = true;
        if (refresh) {
          const float delta = bmx;
          mref[g] += delta;
          if (!first) {
            const float corr = __builtin_amdgcn_exp2f(-delta);
            lsum[g] *= corr;
#pragma unroll
            for (int e = 0; e < HP; ++e) acc[g][e] *= corr;
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[g][r] -= delta;
          if (xlane) qf[g][SX] = -mref[g];
        }
        }
        acc_empty[g] = false;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const float p0 = __builtin_amdgcn_exp2f(sc[g][r]);
          const float p1 = __builtin_amdgcn_exp2f(sc[g][r + 1]);
          sc[g][r] = p0;
          sc[g][r + 1] = p1;
          lsum[g] += f32x2{p0, p1};
        }
      }
      if constexpr (STAMP) {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long n = FFD_STAMP_T();
        st.sm += n - st_a, st_a = n;
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        f32x2 vv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) vv[e] = vb[r % PF][e];
#pragma unroll
        for (int g = 0; g < QG; ++g) {
          const f32x2 pp = f32x2{sc[g][r & ~1], sc[g][(r & ~1) + 1]};  // (adjacent registers of the accumulator)
#pragma unroll
          for (int e = 0; e < HP; ++e) acc[g][e] = (r & 1) ? pk_fma_hi(pp, vv[e], acc[g][e]) : pk_fma_lo(pp, vv[e], acc[g][e]);
        }
        if (r + PF < 16) {
          load_v(r + PF, kbase, vb[r % PF]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (STAMP) {
        __builtin_amdgcn_sched_barrier(0);
        st.pv += FFD_STAMP_T() - st_a;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (STAMP) st.t[5] = FFD_STAMP_T();
    if constexpr (STORE) {
#pragma unroll
      for (int g = 0; g < QG; ++g) {
        float l = lsum[g].x + lsum[g].y;
        l += __shfl_xor(l, 32);
        const float inv = __builtin_amdgcn_rcpf(l);  // (1 ulp; the IEEE division sequence is ten vector instructions per q-tile)
        const int q = 32 * (qt0 + g) + l31;
        float o[2 * HP];
#pragma unroll
        for (int e = 0; e < HP; ++e) {
          float a0 = acc[g][e].x, a1 = acc[g][e].y;
          a0 += __shfl_xor(a0, 32);
          a1 += __shfl_xor(a1, 32);
          o[2 * e] = a0 * inv, o[2 * e + 1] = a1 * inv;
        }
        if (half == 0 && q < L && qt0 + g < QT) {
          float* orow = orow0 + (size_t)q * ostride;
#pragma unroll
          for (int e = 0; e < HD; ++e) orow[e] = o[e];
        }
      }
    } else {
#pragma unroll
      for (int g = 0; g < QG; ++g) {
        rows.mref[g] = mref[g], rows.lsum[g] = lsum[g];
#pragma unroll
        for (int e = 0; e < HP; ++e) rows.acc[g][e] = acc[g][e];
      }
    }
  }
  return rows;
}

// ---- the kernel ----------------------------------------------------------------------------------
//
// SPLIT (small batches, e.g. the benchmark_cache.py harness at batch 1: B*H workgroups would leave most of the chip
// idle and every wave walking 3 q-tiles x 6 key tiles in sequence): `qsplit` workgroups per (sample, head), each
// projecting the whole head but attending only nwaves/kspl q-tiles, with the key range of a q-tile cut into `kspl`
// pieces over the waves (flash-decoding).  The pieces (reference exponent, row sum, unnormalised output) meet in
// LDS and are merged in piece order, so the result does not depend on timing.
// KVQ (split form with the kv | q pack, NCT = 2): tile 0 holds the head's k and v features, tile 1 its q features, and a
// workgroup projects tile 1 only for the tokens of its own q-tiles -- the other q-tiles' workgroups project theirs.
// SB (static bound; launches without K/V tables only): the layer's weights bound every score within T
// (LayerWeights::attn_bounded), so the norm words, head_norms and the barrier behind it are not there and the attention
// phase is the BOUNDED one.
template <int D, int HD, int QG, int NCT, bool SPLIT = false, bool STAMP = false, bool KVQ = false, bool SB = false>
__global__ __launch_bounds__(256, (SPLIT && NCT >= 2 ? 2 : QG <= 2 ? 4 : 3)) void k_qkv_attention(
    const float* __restrict__ x, const float* __restrict__ awp, const float* __restrict__ kt,
    const float* __restrict__ vt, float* __restrict__ kt_out, float* __restrict__ vt_out, float* __restrict__ out,
    int B, int L, int n_own, int q_only, int qsplit, int kspl, unsigned long long* __restrict__ stamp) {
  WaveStamps st;
  if constexpr (STAMP) st.begin();
  constexpr int H = D / HD;
  constexpr int KST = HeadDims<HD>::KST;
  constexpr int C16 = D / 16;           // full 16-wide k chunks
  constexpr int REM = (D % 16) / 4;     // remaining k-steps (k = 16*C16 + 4 i + q)
  constexpr int S4 = (D + 15) / 16;     // float4 groups of packed weight per (h, ct)
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  int b, h, qs = 0;
  {
    int pair = blockIdx.x;
    if constexpr (SPLIT) qs = pair % qsplit, pair /= qsplit;
    xcd_sample_group(pair, B, H, b, h);
  }
  const int KT = (L + 31) >> 5;
  const int Lp = KT * 32;
  // row stride of the LDS images: a compile-time 516 in the four-q-tiles-per-wave instance (launched for KT = 16 only), so
  // that its LDS addresses are per-lane bases + immediate offsets; the run-time Lp elsewhere
  // (+ 4: a stride that is a multiple of 64 floats puts the 16 feature rows a projection tile stores into the same banks)
  constexpr int LSC = (QG == 4 && !SPLIT) ? 516 : 0;
  const int LS = LSC ? LSC : Lp + 4;
  float* vs = lds;                               // V   [Lp][8]
  float* kts = vs + (size_t)LS * 8;              // K^T [2*KST][LS]
  float* qts = kts + (size_t)2 * KST * LS;       // Q^T [2*KST][LS]   (already scaled by log2(e)/sqrt(hd))
  constexpr int PS = 2 + 2 * HeadDims<HD>::HP;  // SPLIT partials per query row: reference exponent, row sum, output
  unsigned* nrm = reinterpret_cast<unsigned*>(lds + HeadDims<HD>::floats(LS) + (SPLIT ? 4 * 32 * PS : 0));  // see head_norms
  if constexpr (!SB) {
    if (threadIdx.x < 2) nrm[threadIdx.x] = 0u;  // (ordered before head_norms by the barrier behind the projection)
  }

  if constexpr (HD % 2 == 1) {  // odd head dims read one pad row / pad column: keep them zero
    for (int idx = threadIdx.x; idx < LS * (8 + 4 * KST); idx += blockDim.x) vs[idx] = 0.f;
    __syncthreads();
  }

  // ------------------------------------------------------------------ phase 1: projection
  {
    const int n = lane & 15, qq = lane >> 4;
    // One head of head_dim 6 is 18 features = one 16-wide tile + 2 (v[4], v[5]).  A second tile for those two would be
    // seven eighths padding (576 matrix cycles per 16 tokens); instead every lane, which holds 18 of its token's 72 x
    // values as A operand anyway, forms their partial dot products with the vector ALU (36 FMAs) and the four lanes of
    // a token add theirs up (two xor-shuffles): ~180 cycles.  k order differs from the MFMA chain: rounding-level, in
    // these two features only.
    // (instances with >= 3 q-tiles per wave only: the others are built for 4 waves per SIMD = 128 registers, where the
    //  36 weight registers of the two columns would spill)
    constexpr bool VREM = HD == 6 && NCT == 2 && QG >= 3;
    constexpr int NCTM = VREM ? 1 : NCT;  // feature tiles on the matrix core
    float4 wf[NCTM][S4];
    const float4* Wq = reinterpret_cast<const float4*>(awp) + (size_t)h * NCT * S4 * 64;
#pragma unroll
    for (int ct = 0; ct < NCTM; ++ct)
#pragma unroll
      for (int j = 0; j < S4; ++j) wf[ct][j] = Wq[((size_t)ct * S4 + j) * 64 + lane];
    float4 w16[VREM ? C16 : 1], w17[VREM ? C16 : 1];  // the second tile's columns n = 0, 1 for this lane's k subset (qq)
    float2 w16r = {0.f, 0.f}, w17r = {0.f, 0.f};      // ... and its <= 2 remainder k-steps
    const float* abp = awp + (size_t)H * NCT * S4 * 256 + (size_t)h * NCT * 16;
    float b16 = 0.f, b17 = 0.f;
    if constexpr (VREM) {
#pragma unroll
      for (int j = 0; j < C16; ++j) w16[j] = Wq[((size_t)S4 + j) * 64 + 16 * qq], w17[j] = Wq[((size_t)S4 + j) * 64 + 16 * qq + 1];
      static_assert(!VREM || REM <= 2, "remainder k-steps of the two vector-ALU columns");
      if constexpr (REM > 0) {
        w16r = *reinterpret_cast<const float2*>(&Wq[((size_t)S4 + S4 - 1) * 64 + 16 * qq]);
        w17r = *reinterpret_cast<const float2*>(&Wq[((size_t)S4 + S4 - 1) * 64 + 16 * qq + 1]);
      }
      b16 = abp[16], b17 = abp[17];
    }
    float bias[NCTM];
    // where this lane's feature (16 ct + n) goes, worked out once: float index of token 0 in the LDS images -- Q^T / K^T
    // rows take a lane's four tokens as one float4, V rows ([token][8]) as four scalars 8 floats apart; -1 = no feature
    int sbase[NCTM];
    bool sv[NCTM];
#pragma unroll
    for (int ct = 0; ct < NCTM; ++ct) {
      bias[ct] = abp[ct * 16 + n];
      const int fi = 16 * ct + n;
      int reg = fi / HD, e = fi - reg * HD;
      int kind = q_only ? (fi < HD ? 0 : 3) : (reg > 2 ? 3 : reg);  // 0 q, 1 k, 2 v, 3 none
      if constexpr (KVQ) {
        static_assert(!KVQ || (SPLIT && NCT == 2 && 2 * HD <= 16), "kv | q pack");
        kind = ct == 0 ? (n < HD ? 1 : n < 2 * HD ? 2 : 3) : (n < HD ? 0 : 3);
        e = ct == 0 ? (n < HD ? n : n - HD) : n;
      }
      sv[ct] = kind == 2;
      sbase[ct] = kind == 3 ? -1 : kind == 0 ? LS * 8 + 2 * KST * LS + e * LS : kind == 1 ? LS * 8 + e * LS : e;
    }
    const float* xb = x + (size_t)b * L * D;
    const int TT = Lp >> 4;  // every row of the LDS images gets a (finite) value
    // token tiles [tt0, tt1) this workgroup projects: all of them -- except on a pure cache hit in the split form, where
    // K and V come from the tables and a workgroup needs q for ITS q-tiles only (the other workgroups of the head
    // project theirs): 2 of 12 tiles at batch 1
    int tt0 = 0, tt1 = TT;
    int ot0 = 0, ot1 = TT;  // token tiles of this workgroup's own q-tiles (KVQ: only they get tile 1 = q)
    if constexpr (SPLIT) {
      const int qpw = nwaves / kspl;
      ot0 = min(2 * qs * qpw, TT), ot1 = min(ot0 + 2 * qpw, TT);
      if (q_only) tt0 = ot0, tt1 = ot1;
    }
    auto load_x = [&](int tt, float4(&xa)[C16 > 0 ? C16 : 1], float(&xr)[REM > 0 ? REM : 1]) {
      int tok = 16 * tt + n;
      if (tok >= L) tok = L - 1;  // padded tokens repeat the last row: finite values that are masked / never stored
      const float* xp = xb + (size_t)tok * D;
#pragma unroll
      for (int j = 0; j < C16; ++j) xa[j] = *reinterpret_cast<const float4*>(xp + 16 * j + 4 * qq);
#pragma unroll
      for (int i = 0; i < REM; ++i) xr[i] = xp[16 * C16 + 4 * i + qq];
    };
    // x tiles are requested PFX tiles ahead: one tile's MFMAs take ~0.5 us, a global load 1-2 us
    constexpr int PFX = VREM ? 3 : 4;  // (three with the two vector-ALU columns' weights in registers: no scratch)
    float4 xa[PFX][C16 > 0 ? C16 : 1];
    float xr[PFX][REM > 0 ? REM : 1];
#pragma unroll
    for (int u = 0; u < PFX; ++u)  // unconditional (tile index clamped): conditional loads would force vmcnt(0) waits
      load_x(min(tt0 + wave + u * nwaves, TT - 1), xa[u], xr[u]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (STAMP) st.t[2] = FFD_STAMP_T();
    // Straight-line code (full unroll, forward exits only): a loop back-edge would make the compiler wait for
    // *all* outstanding loads at every tile (vmcnt(0)), which defeats the ring.  MAXT tiles per wave cover
    // L <= 512 with 4 waves.
    constexpr int MAXT = 8;
#pragma unroll
    for (int it = 0; it < MAXT; ++it) {
      const int u = it % PFX;
      const int tt = tt0 + wave + it * nwaves;
      if (tt >= tt1) break;
      f32x4 acc[NCTM];
#pragma unroll
      for (int ct = 0; ct < NCTM; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bool own = !KVQ || (tt >= ot0 && tt < ot1);  // (wave-uniform) the q tile of the kv | q pack: own tokens only
      auto tile_mfmas = [&](auto CTC) {
        constexpr int ct = decltype(CTC)::value;
#pragma unroll
        for (int j = 0; j < C16; ++j) {
          acc[ct] = mfma16(xa[u][j].x, wf[ct][j].x, acc[ct]);
          acc[ct] = mfma16(xa[u][j].y, wf[ct][j].y, acc[ct]);
          acc[ct] = mfma16(xa[u][j].z, wf[ct][j].z, acc[ct]);
          acc[ct] = mfma16(xa[u][j].w, wf[ct][j].w, acc[ct]);
        }
#pragma unroll
        for (int i = 0; i < REM; ++i) {
          const float4 w4 = wf[ct][S4 - 1];
          const float wv = i == 0 ? w4.x : i == 1 ? w4.y : i == 2 ? w4.z : w4.w;
          acc[ct] = mfma16(xr[u][i], wv, acc[ct]);
        }
      };
      if constexpr (KVQ) {
        tile_mfmas(std::integral_constant<int, 0>{});
        if (own) tile_mfmas(std::integral_constant<int, 1>{});
      } else {
#pragma unroll
        for (int j = 0; j < C16; ++j) {
#pragma unroll
          for (int ct = 0; ct < NCTM; ++ct) {
            acc[ct] = mfma16(xa[u][j].x, wf[ct][j].x, acc[ct]);
            acc[ct] = mfma16(xa[u][j].y, wf[ct][j].y, acc[ct]);
            acc[ct] = mfma16(xa[u][j].z, wf[ct][j].z, acc[ct]);
            acc[ct] = mfma16(xa[u][j].w, wf[ct][j].w, acc[ct]);
          }
        }
#pragma unroll
        for (int i = 0; i < REM; ++i) {
#pragma unroll
          for (int ct = 0; ct < NCTM; ++ct) {
            const float4 w4 = wf[ct][S4 - 1];
            const float wv = i == 0 ? w4.x : i == 1 ? w4.y : i == 2 ? w4.z : w4.w;
            acc[ct] = mfma16(xr[u][i], wv, acc[ct]);
          }
        }
      }
      float p16 = 0.f, p17 = 0.f;
      if constexpr (VREM) {  // features 16, 17 of token n over this lane's k subset
#pragma unroll
        for (int j = 0; j < C16; ++j) {
          p16 = fmaf(xa[u][j].x, w16[j].x, p16), p17 = fmaf(xa[u][j].x, w17[j].x, p17);
          p16 = fmaf(xa[u][j].y, w16[j].y, p16), p17 = fmaf(xa[u][j].y, w17[j].y, p17);
          p16 = fmaf(xa[u][j].z, w16[j].z, p16), p17 = fmaf(xa[u][j].z, w17[j].z, p17);
          p16 = fmaf(xa[u][j].w, w16[j].w, p16), p17 = fmaf(xa[u][j].w, w17[j].w, p17);
        }
#pragma unroll
        for (int i = 0; i < REM; ++i) {
          p16 = fmaf(xr[u][i], i == 0 ? w16r.x : w16r.y, p16), p17 = fmaf(xr[u][i], i == 0 ? w17r.x : w17r.y, p17);
        }
      }
      if (it + PFX < MAXT) load_x(min(tt + PFX * nwaves, TT - 1), xa[u], xr[u]);  // refill this slot (clamped, unconditional)
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (VREM) {  // the token's four lanes (k subsets qq = 0 .. 3, 16 lanes apart) add up; qq = 0 stores v[4], v[5]
        p16 += __shfl_xor(p16, 16), p17 += __shfl_xor(p17, 16);
        p16 += __shfl_xor(p16, 32), p17 += __shfl_xor(p17, 32);
        if (qq == 0) *reinterpret_cast<float2*>(vs + (size_t)(16 * tt + n) * 8 + 4) = float2{p16 + b16, p17 + b17};
      }
      const int t0 = 16 * tt + 4 * qq;  // D: lane holds tokens t0 .. t0+3 of feature 16 ct + n
#pragma unroll
      for (int ct = 0; ct < NCTM; ++ct) {
        const float4 o = float4{acc[ct][0] + bias[ct], acc[ct][1] + bias[ct], acc[ct][2] + bias[ct],
                                acc[ct][3] + bias[ct]};
        if (sbase[ct] >= 0 && (ct == 0 || own)) {
          if (!sv[ct]) {
            *reinterpret_cast<float4*>(lds + sbase[ct] + t0) = o;
          } else {
            float* vp = lds + sbase[ct] + t0 * 8;
            vp[0] = o.x, vp[8] = o.y, vp[16] = o.z, vp[24] = o.w;
          }
        }
      }
    }
  }
  if constexpr (STAMP) st.t[3] = FFD_STAMP_T();
  if constexpr (!SB) {
    if (kt != nullptr) fill_from_tables<HD>(vs, kts, LS, kt, vt, h, L, Lp, n_own, q_only, threadIdx.x, blockDim.x);
  }
  __syncthreads();  // the LDS images
  bool bounded = true;
  if constexpr (!SB) {
    {  // (q rows outside the projected token range were never written: they stay out of the bound)
      int jq0 = 0, jq1 = Lp;
      if constexpr (SPLIT) {
        if (q_only || KVQ) {
          const int qpw = nwaves / kspl;
          jq0 = min(32 * qs * qpw, Lp), jq1 = min(jq0 + 32 * qpw, Lp);
        }
      }
      head_norms<HD>(kts, qts, nrm, Lp, LS, threadIdx.x, blockDim.x, jq0, jq1);
    }
    if (kt_out != nullptr && b == 0 && qs == 0)
      publish_kv<HD>(vs, kts, LS, kt_out, vt_out, h, L, n_own, threadIdx.x, blockDim.x);

    __syncthreads();  // the tile norms
    bounded = head_bounded<HD>(nrm);
  }
  if constexpr (STAMP) st.t[4] = FFD_STAMP_T();
  float* orow0 = out + (size_t)b * L * D + h * HD;  // the head's output row for query token q: orow0 + q * D
  if constexpr (SPLIT) {  // one (q-tile, key piece) per wave
    const int qpw = nwaves / kspl, kps = (KT + kspl - 1) / kspl;
    const int qt = qs * qpw + wave / kspl, t_lo = (wave % kspl) * kps;
    int t_hi = min(KT, t_lo + kps);
    if (qt >= KT) t_hi = t_lo;  // ragged last workgroup: an empty piece (every wave reaches the merge)
    const QRows<HD, 1> r = attend_qtiles<HD, 1, STAMP, false, 0, SB>((lds_f32*)vs, (lds_f32*)kts, (lds_f32*)qts, LS, qt, 1,
                                                                 qt + 1, t_lo, t_hi, bounded, L, orow0, D, st);
    const int half = lane >> 5, l31 = lane & 31;
    float* part = lds + HeadDims<HD>::floats(LS);  // [wave][32][PS]
    float l = r.lsum[0].x + r.lsum[0].y;
    l += __shfl_xor(l, 32);
    float o[PS - 2];
#pragma unroll
    for (int e = 0; e < HeadDims<HD>::HP; ++e) {
      float a0 = r.acc[0][e].x, a1 = r.acc[0][e].y;
      o[2 * e] = a0 + __shfl_xor(a0, 32), o[2 * e + 1] = a1 + __shfl_xor(a1, 32);
    }
    if (half == 0) {
      float* pw = part + (size_t)(wave * 32 + l31) * PS;
      pw[0] = (t_lo < t_hi) ? r.mref[0] : -INFINITY;  // an empty piece weighs 2^-inf = 0 in the merge
      pw[1] = l;
#pragma unroll
      for (int e = 0; e < PS - 2; ++e) pw[2 + e] = o[e];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < qpw * 32 * HD; idx += blockDim.x) {
      const int e = idx % HD, ql = (idx / HD) & 31, qi = idx / (HD * 32);
      const int qtile = qs * qpw + qi, q = 32 * qtile + ql;
      if (qtile >= KT || q >= L) continue;
      const float* p0 = part + (size_t)(qi * kspl * 32 + ql) * PS;
      float mx = -INFINITY;
      for (int sp = 0; sp < kspl; ++sp) mx = fmaxf(mx, p0[(size_t)sp * 32 * PS]);
      float lt = 0.f, ot = 0.f;
      for (int sp = 0; sp < kspl; ++sp) {
        const float* pp = p0 + (size_t)sp * 32 * PS;
        const float wgt = __builtin_amdgcn_exp2f(pp[0] - mx);
        lt = fmaf(pp[1], wgt, lt), ot = fmaf(pp[2 + e], wgt, ot);
      }
      orow0[(size_t)q * D + e] = ot / lt;
    }
  } else {
    attend_qtiles<HD, QG, STAMP, true, LSC, SB>((lds_f32*)vs, (lds_f32*)kts, (lds_f32*)qts, LS, wave * QG, nwaves * QG, KT,
                                            0, KT, bounded, L, orow0, D, st);
  }
  if constexpr (STAMP) st.write(stamp, nwaves);
}

// ---- multi-head variant ------------------------------------------------------------------------------
// HPW heads of one sample per workgroup (2 waves per head).  Why: with one head per workgroup every
// workgroup re-reads the sample's x rows and its own weight slice, and the kernel is paced by the L1 request
// rate at workgroup start (measured: ~20k cycles until a wave's second tile vs ~2.3k per tile afterwards).
// Here x is read once for HPW heads, the HPW*3*hd features are packed densely into 16-wide tiles
// (2 heads x 18 = 36 features -> 3 tiles, 75 % useful, vs 18 -> 2 tiles, 56 %), and the weight pack is
// staged once in LDS and read as the MFMA B operand from there.  Two heads = 4 waves, one per SIMD: a 6-wave
// workgroup (3 heads) leaves the CU with a single resident workgroup (two of its waves land on SIMDs 0 and 1,
// so a second one never fits at 3 waves per SIMD) and was slower.
// SB: see k_qkv_attention.
template <int D, int HD, int HPW, int QG, int NCT, bool QO, bool STAMP = false, bool SB = false>
__global__ __launch_bounds__(128 * HPW, 3) void k_qkv_attention_mh(
    const float* __restrict__ x, const float* __restrict__ awp, const float* __restrict__ kt,
    const float* __restrict__ vt, float* __restrict__ kt_out, float* __restrict__ vt_out, float* __restrict__ out,
    int B, int L, int n_own, int q_only, unsigned long long* __restrict__ stamp) {
  WaveStamps st;
  if constexpr (STAMP) st.begin();
  constexpr int H = D / HD;
  constexpr int NG = H / HPW;
  constexpr int KST = HeadDims<HD>::KST;
  constexpr int C16 = D / 16;
  constexpr int REM = (D % 16) / 4;
  constexpr int S4 = (D + 15) / 16;
  constexpr int NW = 2 * HPW;           // waves per workgroup
  constexpr int MAXT = 3;               // token tiles per wave: Lp <= 192 -> 12 tiles over >= 4 waves
  // Two heads of head_dim 6 are 36 features: two 16-wide tiles + 4 (head 1's v[2..5]).  A third tile would be three
  // quarters padding; the four features are partial dot products over the 18 of its token's 72 x values each lane holds
  // as A operand anyway, added up over the token's four lanes (two xor-shuffles).  They run on v_mfma_f32_4x4x1_16b_f32
  // with those x registers as B operand as they are (18 steps = 144 matrix cycles per 16 tokens, 18 weight registers);
  // as vector-ALU FMAs (round 4) they were 72 v_fmac = 288 cycles and 72 weight registers, and fp32 vector time adds to
  // matrix time on a SIMD.  (Round 3's 4x4x1 form was lane = token and read every x row a second time: dropped.)
  constexpr bool REMV = HD == 6 && HPW == 2 && NCT == 3;
  constexpr int NCTM = REMV ? 2 : NCT;  // 16-wide feature tiles on the 16x16x4 form
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int b, hg;
  xcd_sample_group(blockIdx.x, B, NG, b, hg);
  const int KT = (L + 31) >> 5;
  const int Lp = KT * 32;
  // the LDS images have a COMPILE-TIME row stride (a wave owns QG q-tiles, a head two waves: Lp <= LS): every LDS address
  // below is one per-lane base + immediate offsets instead of multiplications by a run-time Lp
  constexpr int LS = 64 * QG + 4;  // (+ 4: see k_qkv_attention)
  constexpr int RS = HeadDims<HD>::floats(LS);                 // floats per head region: V | K^T | Q^T
  float4* wl = reinterpret_cast<float4*>(lds + (size_t)HPW * RS);  // weight pack [NCT][S4][64] float4
  constexpr int fph = QO ? HD : 3 * HD;                        // features per head in this pack (QO == q_only)
  if constexpr (!SB) {
    if (threadIdx.x < 2 * HPW)  // the heads' norm words (ordered before head_norms by the barriers of the projection)
      reinterpret_cast<unsigned*>(lds + (size_t)HPW * RS + (size_t)NCT * S4 * 256)[threadIdx.x] = 0u;
  }

  // ------------------------------------------------------------------ phase 1: projection
  {
    const int n = lane & 15, qq = lane >> 4;
    const float* xb = x + (size_t)b * L * D;
    const int TT = Lp >> 4;
    auto load_x = [&](int tt, float4(&xa)[C16 > 0 ? C16 : 1], float(&xr)[REM > 0 ? REM : 1]) {
      int tok = 16 * tt + n;
      if (tok >= L) tok = L - 1;
      const float* xp = xb + (size_t)tok * D;
#pragma unroll
      for (int j = 0; j < C16; ++j) xa[j] = *reinterpret_cast<const float4*>(xp + 16 * j + 4 * qq);
#pragma unroll
      for (int i = 0; i < REM; ++i) xr[i] = xp[16 * C16 + 4 * i + qq];
    };
    // every x tile of this wave is requested up front (unconditional, clamped), then the weights are staged
    float4 xa[MAXT][C16 > 0 ? C16 : 1];
    float xr[MAXT][REM > 0 ? REM : 1];
#pragma unroll
    for (int u = 0; u < MAXT; ++u) load_x(min(wave + u * NW, TT - 1), xa[u], xr[u]);
    {
      const float4* Wq = reinterpret_cast<const float4*>(awp) + (size_t)hg * NCT * S4 * 64;
      for (int i = threadIdx.x; i < NCT * S4 * 64; i += 64 * NW) wl[i] = Wq[i];
      if constexpr (HD % 2 == 1) {  // odd head dims read one pad row / pad column: keep them zero
        for (int idx = threadIdx.x; idx < HPW * RS; idx += 64 * NW) lds[idx] = 0.f;
      }
    }
    const float* abp = awp + (size_t)NG * NCT * S4 * 256 + (size_t)hg * NCT * 16;
    float bias[NCTM];
    // where this lane's feature (16 ct + n) goes, worked out once: float index of token 0 in the LDS images -- Q^T / K^T
    // rows take a lane's four tokens as one float4, V rows ([token][8]) as four scalars 8 floats apart; -1 = no feature
    int sbase[NCTM];
    StorePlan sp[NCTM];
#pragma unroll
    for (int ct = 0; ct < NCTM; ++ct) {
      bias[ct] = abp[ct * 16 + n];
      const int fi = 16 * ct + n;
      const int hh = fi / fph, f = fi - hh * fph;
      const int reg = f / HD, e = f - reg * HD;
      sbase[ct] = hh >= HPW ? -1
                  : hh * RS + (reg == 0 ? LS * 8 + 2 * KST * LS + e * LS : reg == 1 ? LS * 8 + e * LS : e);
      sp[ct].init(lds, sbase[ct], reg == 2, 16 * wave + 4 * qq, 16 * NW);
    }
    __syncthreads();
    if constexpr (STAMP) st.t[2] = FFD_STAMP_T();
    // The third tile's columns 0 .. 3 as the A operand of the 4x4x1 form: block b = lane >> 2 pairs A[lane 4 b + i] with
    // B[lane 4 b + j], and the four lanes of a block share qq (= b >> 2), so with A = column (lane & 3) over this lane's k
    // subset and B = the x values the lane holds anyway, output register i of lane (qq, n) is the partial dot product
    // of feature 32 + i and token n over qq's k values: one k per step, in the order of the former FMA chain.
    float wrem[REMV ? 4 * C16 + REM : 1];
    float bvv[REMV ? 4 : 1];
    if constexpr (REMV) {
      static_assert(!REMV || REM <= 4, "remainder k-steps come from one staged float4");
#pragma unroll
      for (int j = 0; j < C16; ++j) {
        const float4 w4 = wl[(2 * S4 + j) * 64 + 16 * qq + (lane & 3)];
        wrem[4 * j] = w4.x, wrem[4 * j + 1] = w4.y, wrem[4 * j + 2] = w4.z, wrem[4 * j + 3] = w4.w;
      }
      if constexpr (REM > 0) {
        const float4 r4 = wl[(2 * S4 + S4 - 1) * 64 + 16 * qq + (lane & 3)];
#pragma unroll
        for (int i = 0; i < REM; ++i) wrem[4 * C16 + i] = i == 0 ? r4.x : i == 1 ? r4.y : i == 2 ? r4.z : r4.w;
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) bvv[f] = abp[2 * 16 + f];
    }
#pragma unroll
    for (int it = 0; it < MAXT; ++it) {
      const int tt = wave + it * NW;
      if (tt >= TT) break;
      if constexpr (REMV) {
        // all of a tile's 4x4x1 steps together (switching MFMA forms step by step costs 47 cycles each: ffd_ffn_rows.hip)
        f32x4 pr = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < C16; ++j) {
          pr = __builtin_amdgcn_mfma_f32_4x4x1f32(wrem[4 * j], xa[it][j].x, pr, 0, 0, 0);
          pr = __builtin_amdgcn_mfma_f32_4x4x1f32(wrem[4 * j + 1], xa[it][j].y, pr, 0, 0, 0);
          pr = __builtin_amdgcn_mfma_f32_4x4x1f32(wrem[4 * j + 2], xa[it][j].z, pr, 0, 0, 0);
          pr = __builtin_amdgcn_mfma_f32_4x4x1f32(wrem[4 * j + 3], xa[it][j].w, pr, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < REM; ++i) pr = __builtin_amdgcn_mfma_f32_4x4x1f32(wrem[4 * C16 + i], xr[it][i], pr, 0, 0, 0);
        float pv[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {  // the token's four lanes (k subsets qq = 0 .. 3, 16 lanes apart) add up
          float p = pr[f];
          p += __shfl_xor(p, 16);
          p += __shfl_xor(p, 32);
          pv[f] = p + bvv[f];
        }
        if (qq == 0) {  // head 1 of the workgroup, v[2 .. 5] of token 16 tt + n
          float* vp = lds + RS + (16 * tt + n) * 8 + 2;
          *reinterpret_cast<float2*>(vp) = float2{pv[0], pv[1]};
          *reinterpret_cast<float2*>(vp + 2) = float2{pv[2], pv[3]};
        }
      }
      f32x4 acc[NCTM];
#pragma unroll
      for (int ct = 0; ct < NCTM; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < C16; ++j) {
#pragma unroll
        for (int ct = 0; ct < NCTM; ++ct) {
          const float4 w4 = wl[(ct * S4 + j) * 64 + lane];
          acc[ct] = mfma16(xa[it][j].x, w4.x, acc[ct]);
          acc[ct] = mfma16(xa[it][j].y, w4.y, acc[ct]);
          acc[ct] = mfma16(xa[it][j].z, w4.z, acc[ct]);
          acc[ct] = mfma16(xa[it][j].w, w4.w, acc[ct]);
        }
      }
      if constexpr (REM > 0) {
#pragma unroll
        for (int ct = 0; ct < NCTM; ++ct) {
          const float4 w4 = wl[(ct * S4 + S4 - 1) * 64 + lane];
#pragma unroll
          for (int i = 0; i < REM; ++i) {
            const float wv = i == 0 ? w4.x : i == 1 ? w4.y : i == 2 ? w4.z : w4.w;
            acc[ct] = mfma16(xr[it][i], wv, acc[ct]);
          }
        }
      }
      // D: lane holds tokens 16 tt + 4 qq .. + 3 of feature 16 ct + n
#pragma unroll
      for (int ct = 0; ct < NCTM; ++ct) {
        if (sbase[ct] >= 0)
          sp[ct].store(acc[ct][0] + bias[ct], acc[ct][1] + bias[ct], acc[ct][2] + bias[ct], acc[ct][3] + bias[ct]);
        sp[ct].next_tile();
      }
    }
  }
  if constexpr (STAMP) st.t[3] = FFD_STAMP_T();
  // this wave's head for the rest of the kernel
  const int hh = wave >> 1, gw = wave & 1;
  const int h = hg * HPW + hh;
  float* vs = lds + (size_t)hh * RS;
  float* kts = vs + LS * 8;
  float* qts = kts + 2 * KST * LS;
  if constexpr (!SB) {
    if (kt != nullptr) fill_from_tables<HD>(vs, kts, LS, kt, vt, h, L, Lp, n_own, q_only, gw * 64 + lane, 128);
  }
  __syncthreads();  // the LDS images
  bool bounded = true;
  if constexpr (!SB) {
    unsigned* nrm = reinterpret_cast<unsigned*>(lds + (size_t)HPW * RS + (size_t)NCT * S4 * 256) + 2 * hh;  // this head's pair, see head_norms
    head_norms<HD>(kts, qts, nrm, Lp, LS, gw * 64 + lane, 128);
    if (kt_out != nullptr && b == 0) publish_kv<HD>(vs, kts, LS, kt_out, vt_out, h, L, n_own, gw * 64 + lane, 128);

    __syncthreads();  // the tile norms
    bounded = head_bounded<HD>(nrm);
  }
  if constexpr (STAMP) st.t[4] = FFD_STAMP_T();
  attend_qtiles<HD, QG, STAMP, true, LS, SB>((lds_f32*)vs, (lds_f32*)kts, (lds_f32*)qts, LS, gw * QG, 2 * QG, KT, 0, KT,
                                             bounded, L, out + (size_t)b * L * D + h * HD, D, st);
  if constexpr (STAMP) st.write(stamp, NW);
}

template <int D, int HD, int HPW, int QG, int NCT, bool QO>
static hipError_t launch_mh_t(const AttnArgs& a, int q_only, hipStream_t s) {
  constexpr int S4 = (D + 15) / 16;
  const int KT = (a.L + 31) / 32;
  const size_t lds = (HPW * HeadDims<HD>::floats(64 * QG + 4) + (size_t)NCT * S4 * 256 + (size_t)HPW * 2) * sizeof(float);
  if (cdiv(2 * KT, 2 * HPW) > 3 || cdiv(KT, 2) > QG) return hipErrorInvalidValue;  // <= 3 token tiles, one q-group per wave
  if (a.static_bound && (QO || a.kt != nullptr)) return hipErrorInvalidValue;  // the static form is the full pack's, without tables
  auto go = [&](auto kern, unsigned long long* stamp) {
    hipLaunchKernelGGL(kern, dim3(a.B * (D / HD / HPW)), dim3(128 * HPW), lds, s, a.x, a.pack, a.kt, a.vt, a.kt_out, a.vt_out,
                       a.out, a.B, a.L, a.n_own, q_only, stamp);
    return hipGetLastError();
  };
  if constexpr (D == 72 && HD == 6) {  // (the stamped twins exist for the headline shape only)
    if (a.stamp != nullptr) {
      if constexpr (!QO) {
        if (a.static_bound) return go(k_qkv_attention_mh<D, HD, HPW, QG, NCT, QO, true, true>, a.stamp);
      }
      return go(k_qkv_attention_mh<D, HD, HPW, QG, NCT, QO, true>, a.stamp);
    }
  }
  if (a.stamp != nullptr) return hipErrorInvalidValue;
  if (q_only != (QO ? 1 : 0)) return hipErrorInvalidValue;
  if constexpr (!QO) {
    if (a.static_bound) return go(k_qkv_attention_mh<D, HD, HPW, QG, NCT, QO, false, true>, nullptr);
  }
  return go(k_qkv_attention_mh<D, HD, HPW, QG, NCT, QO>, nullptr);
}

// 2 heads per workgroup, 2 waves per head: L <= 192 (<= 3 q-tiles per wave, 12 token tiles over 4 waves)
template <int D, int HD>
static hipError_t launch_mh2(const AttnArgs& a, int q_only, int qg, hipStream_t s) {
  constexpr int NF = (2 * 3 * HD + 15) / 16, NQ = (2 * HD + 15) / 16;
#define FFD_MH(g) \
  if (qg == g) return q_only ? launch_mh_t<D, HD, 2, g, NQ, true>(a, 1, s) : launch_mh_t<D, HD, 2, g, NF, false>(a, 0, s);
  FFD_MH(1) FFD_MH(2) FFD_MH(3)
#undef FFD_MH
  return hipErrorInvalidValue;
}

// FULL: the q | k | v pack (the only one with a static-bound instance)
template <int D, int HD, int QG, int NCT, bool FULL>
static hipError_t launch_t(const AttnArgs& a, int q_only, hipStream_t s) {
  const int KT = (a.L + 31) / 32;
  const size_t lds = (HeadDims<HD>::floats(KT * 32 + 4) + (size_t)2 * KT) * sizeof(float);
  int nwaves = cdiv(KT, QG);
  if (nwaves > 4) nwaves = 4;
  if (cdiv(2 * KT, nwaves) > 8) return hipErrorInvalidValue;  // the projection loop is unrolled for <= 8 token tiles per wave
  if (a.static_bound && (!FULL || q_only || a.kt != nullptr)) return hipErrorInvalidValue;
  auto go = [&](auto kern, unsigned long long* stamp) {
    hipLaunchKernelGGL(kern, dim3(a.B * (D / HD)), dim3(64 * nwaves), lds, s, a.x, a.pack, a.kt, a.vt, a.kt_out, a.vt_out,
                       a.out, a.B, a.L, a.n_own, q_only, 1, 1, stamp);
    return hipGetLastError();
  };
  if constexpr (D == 72 && HD == 6 && NCT == 2) {  // (the stamped twins exist for the headline model's full pack only)
    if (a.stamp != nullptr) {
      if (a.static_bound) return go(k_qkv_attention<D, HD, QG, NCT, false, true, false, true>, a.stamp);
      return go(k_qkv_attention<D, HD, QG, NCT, false, true>, a.stamp);
    }
  }
  if (a.stamp != nullptr) return hipErrorInvalidValue;
  if constexpr (FULL) {
    if (a.static_bound) return go(k_qkv_attention<D, HD, QG, NCT, false, false, false, true>, nullptr);
  }
  return go(k_qkv_attention<D, HD, QG, NCT>, nullptr);
}

// small batches: 4 waves per workgroup, 4 / kspl q-tiles per workgroup, the key range of each cut into kspl pieces
template <int D, int HD, int NCT, bool KVQ = false, bool FULL = false>
static hipError_t launch_split_t(const AttnArgs& a, int q_only, int kspl, hipStream_t s) {
  const int KT = (a.L + 31) / 32;
  if (cdiv(2 * KT, 4) > 8 || (kspl != 1 && kspl != 2 && kspl != 4)) return hipErrorInvalidValue;
  const int qsplit = cdiv(KT, 4 / kspl);
  const size_t lds =
      (HeadDims<HD>::floats(KT * 32 + 4) + (size_t)4 * 32 * (2 + 2 * HeadDims<HD>::HP) + (size_t)2 * KT) * sizeof(float);
  if (a.static_bound && (!FULL || q_only || a.kt != nullptr)) return hipErrorInvalidValue;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(a.B * (D / HD) * qsplit), dim3(256), lds, s, a.x, a.pack, a.kt, a.vt, a.kt_out, a.vt_out,
                       a.out, a.B, a.L, a.n_own, q_only, qsplit, kspl, (unsigned long long*)nullptr);
    return hipGetLastError();
  };
  if constexpr (FULL) {
    if (a.static_bound) return go(k_qkv_attention<D, HD, 1, NCT, true, false, KVQ, true>);
  }
  return go(k_qkv_attention<D, HD, 1, NCT, true, false, KVQ>);
}

// Key pieces per q-tile of the small-batch split form, 0 when the one-workgroup-per-head(-pair) kernels run: the
// split form projects a head once per q-split, which only pays while the chip is not full.
int qkv_attention_small_split(int B, int H, int L) {
  if (g_attn_small == 0 || L > 512) return 0;
  if (g_attn_small == 2 || g_attn_small == 4) return g_attn_small;
  const int QT = (L + 31) / 32;
  // tools/sweep_small.py (ECG, H = 12, 6 q-tiles): four key pieces win while the grid stays under ~5/8 of the CUs
  // (B <= 2), two pieces up to ~5/4 (B <= 8); beyond that the repeated projection costs more than the idle CUs
  if (8L * B * H * QT <= 5L * num_cus()) return 4;
  if (4L * B * H * cdiv(QT, 2) <= 5L * num_cus()) return 2;
  return 0;
}

// q-tiles per wave (the group shares every K^T / V read) of the one-workgroup-per-head kernels at QT q-tiles: of
// k_qkv_attention (fused), else of k_attention_mfma, which has no instance of four
int attn_qg(int QT, int hd, bool fused) {
  if (QT == 1) return 1;
  if (QT % 3 == 0) return 3;
  // long sequences: four q-tiles per wave (L = 512: 2422 -> 2286 us against two per wave; hd = 8 has no such instance)
  if (fused && hd <= 6 && QT % 4 == 0 && QT >= 16) return 4;
  return 2;
}

template <int D, int HD>
static hipError_t launch_dh(const AttnArgs& a, int q_only, int kspl, int qg, hipStream_t s) {
  constexpr int NCTF = (3 * HD + 15) / 16;
  if (kspl) {
    if (a.stamp != nullptr) return hipErrorInvalidValue;  // (no stamped twin of the split form)
    if constexpr (2 * HD <= 16 && 3 * HD > 16) {  // (q_only == 2: the caller handed over the kv | q pack)
      if (q_only == 2) return launch_split_t<D, HD, 2, true, true>(a, 0, kspl, s);
    }
    if (q_only == 2) return hipErrorInvalidValue;
    return q_only ? launch_split_t<D, HD, 1>(a, 1, kspl, s) : launch_split_t<D, HD, NCTF, false, true>(a, 0, kspl, s);
  }
  if (q_only == 2) return hipErrorInvalidValue;  // the kv | q pack is the split form's only
  if (q_only && a.stamp != nullptr) return hipErrorInvalidValue;
  // (instances in the order they were first named in: the device code keeps its layout)
#define FFD_QG(g, nct) if (qg == g) return launch_t<D, HD, g, nct, false>(a, q_only, s);
  if (q_only) {
    FFD_QG(1, 1) FFD_QG(3, 1)
    if constexpr (HD <= 6) {
      FFD_QG(4, 1)
    }
    FFD_QG(2, 1)
    return hipErrorInvalidValue;
  }
#undef FFD_QG
#define FFD_QG(g, nct) if (qg == g) return launch_t<D, HD, g, nct, true>(a, q_only, s);
  FFD_QG(2, NCTF) FFD_QG(1, NCTF) FFD_QG(3, NCTF)
  if constexpr (HD <= 6) {  // (hd = 8 would spill at four query groups)
    FFD_QG(4, NCTF)
  }
#undef FFD_QG
  return hipErrorInvalidValue;
}

// (d_model, head_dim) pairs with a fused kernel, X2: with a two-heads-per-workgroup instance as well; anything else
// keeps the two-kernel path.
#define FFD_QKV_LIST(X, X2) X2(72, 6) X2(60, 5) X(24, 6) X(8, 2) X(64, 8) X2(48, 4) X(32, 8) X(16, 4) X(24, 3)
#define FFD_QKV_IS(dd, hh) if (D == dd && hd == hh) return true;
#define FFD_QKV_SKIP(dd, hh)

bool qkv_attention_supported(int D, int hd) {
  FFD_QKV_LIST(FFD_QKV_IS, FFD_QKV_IS)
  return false;
}
static bool qkv_attention_two_heads(int D, int hd) {
  FFD_QKV_LIST(FFD_QKV_SKIP, FFD_QKV_IS)
  return false;
}

// heads per workgroup of the one-workgroup-per-head(-pair) kernels for this shape (the caller passes the matching pack)
int qkv_attention_hpw(int D, int hd, int L) {
  return (g_attn_hpw == 1 || !qkv_attention_two_heads(D, hd) || L > 192) ? 1 : 2;
}

hipError_t launch_qkv_attention(const AttnArgs& a, int D, int hd, int hpw, int q_only, int kspl, int qg, hipStream_t s) {
  if (a.B <= 0) return hipSuccess;
  if (hpw == 2) {
#define FFD_QA2(dd, hh) if (D == dd && hd == hh) return launch_mh2<dd, hh>(a, q_only, qg, s);
    FFD_QKV_LIST(FFD_QKV_SKIP, FFD_QA2)
#undef FFD_QA2
    return hipErrorInvalidValue;
  }
#define FFD_QA(dd, hh) if (D == dd && hd == hh) return launch_dh<dd, hh>(a, q_only, kspl, qg, s);
  FFD_QKV_LIST(FFD_QA, FFD_QA)
#undef FFD_QA
  return hipErrorInvalidValue;
}

}  // namespace ffd
