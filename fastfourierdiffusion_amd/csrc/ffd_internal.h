// Internal declarations shared by the libffd translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ffd.h"

namespace ffd {

constexpr int WAVE = 64;

// d_model / head_dim values with compiled kernels (every d % 4 == 0, d <= 72; hd <= 8)
#define FFD_D_LIST(X) X(8) X(16) X(24) X(32) X(48) X(60) X(64) X(72)
#define FFD_HD_LIST(X) X(2) X(3) X(4) X(5) X(6) X(8)

// ---- MFMA f32 16x16x4 fragment conventions (cdna_hip_programming.md §3) ----
//   A operand: lane l holds A[i = l & 15][k = l >> 4]
//   B operand: lane l holds B[k = l >> 4][j = l & 15]
//   C/D      : lane l, reg r holds D[i = 4 * (l >> 4) + r][j = l & 15]
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

constexpr __host__ __device__ int cdiv(int a, int b) { return (a + b - 1) / b; }

// float4 access through p is allowed (nullptr: an absent array)
inline bool ptr16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// relu as ONE vector instruction (v_max_i32): max of the bit pattern, as a signed integer, with 0.  Negative floats
// and -0.0 are negative integers -> +0.0; +0.0, positive floats and +inf are themselves: for every non-NaN x the bits
// of fmaxf(x, 0).  (A float max / med3 of an MFMA result costs two: hipcc cannot prove the accumulator canonical and
// puts a quieting v_max_f32 x, x, x in front, and on this chip a vector instruction in a matrix-bound loop is matrix
// time lost.  Plain C++ on purpose: behind an inline-asm v_max_f32 the compiler no longer inserts the MFMA-write ->
// VALU-read wait states.)
__device__ __forceinline__ float relu_bits(float x) {
  const int i = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, i > 0 ? i : 0);
}

// ---- Philox4x32-10 + Box-Muller: the on-device N(0,1) / U[0,1) draws (SDE step, prior, score-matching loss) ----
struct U4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    // one 32 x 32 -> 64 multiply per product (v_mad_u64_u32) instead of a mul_hi / mul_lo pair: the generator is the
    // ALU floor of the noise-drawing kernels (the prior writes 4 B per element and nothing else)
    const uint64_t p0 = (uint64_t)M0 * c.x, p1 = (uint64_t)M1 * c.z;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    U4 n = {hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    c = n;
    k0 += W0;
    k1 += W1;
  }
  return c;
}

// Two N(0,1) draws from two 32-bit words.  The hardware transcendentals (v_log_f32 = log2, v_sin_f32 / v_cos_f32 take
// their argument in revolutions, i.e. u2 itself) keep the generator off the critical path of the HBM-bound step
// kernel: the library logf / sincosf cost ~10x the instructions and made the step ALU-bound (2.8 TB/s).
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0,1)
  const float u2 = ((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));  // sqrt(-2 ln u1)
  z0 = r * __builtin_amdgcn_cosf(u2);
  z1 = r * __builtin_amdgcn_sinf(u2);
}

// N(0,1) for global element index g at (seed, stream tag `step`): slot g&3 of Philox(counter g>>2).
__device__ __forceinline__ void normal4(uint64_t g4, uint64_t seed, uint32_t step, float out[4]) {
  U4 c = {(uint32_t)g4, (uint32_t)(g4 >> 32), step, 0x46464446u /* "FFDF" */};
  U4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  box_muller(r.x, r.y, out[0], out[1]);
  box_muller(r.z, r.w, out[2], out[3]);
}

// the (up to) 4 draws of elements i0 .. i0+3 (global index elem_offset + i0, any alignment), or injected ones
__device__ __forceinline__ void load_normals(const float* z, size_t i0, int n, uint64_t seed, uint64_t elem_offset,
                                             uint32_t step, float zz[4]) {
  if (z) {
    for (int j = 0; j < n; ++j) zz[j] = z[i0 + j];
    return;
  }
  uint64_t g0 = elem_offset + i0;
  float a[4], b[4] = {0.f, 0.f, 0.f, 0.f};
  normal4(g0 >> 2, seed, step, a);
  const int sh = (int)(g0 & 3);
  if (sh) normal4((g0 >> 2) + 1, seed, step, b);
  // zz[j] = (a | b)[sh + j] as selects on static indices (indexed by sh the two arrays lived in scratch: 48 B per lane)
  const float c[7] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2]};
#pragma unroll
  for (int j = 0; j < 4; ++j) zz[j] = sh == 0 ? c[j] : sh == 1 ? c[j + 1] : sh == 2 ? c[j + 2] : c[j + 3];
}

// Sum over a 256-thread workgroup as a fixed-order fp64 tree in LDS (red: 256 doubles); every thread gets the total
__device__ __forceinline__ double block_sum(double v, double* red) {  // fixed-order tree over 256 threads
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// ---- ffd_tune knobs: each a thread_local int (a thread's knobs select the kernels of the launches it makes; a new
// thread starts from the defaults).  I(key, variable, default, accepted values of v); B(key, variable, default): any
// value, stored as 0 / 1.  ffd_tune, ffd_tune_get, "reset" and the definitions are generated from this table.
#define FFD_KNOBS(I, B)                                                                                                 \
  I("ffn_mb", g_ffn_mb_override, 0, v >= 0 && v <= 4)     /* k_ffn_ln tile height 16 x 1 / 2 / 3 / 4 rows forced; 0 heuristic */ \
  I("ffn_height", g_ffn_height, 1, v >= 0 && v <= 2)      /* 32- / 48-row k_ffn_ln tiles (ffn_height_plan): 0 off | 1 one launch | 2 behind k_linear_res_ln */ \
  I("ffn_persist", g_ffn_persist, 1, v >= 0 && v <= 8)    /* k_ffn_ln MB >= 4: 0 a workgroup per tile; n: persistent grid of n x the resident workgroups */ \
  B("ffn_rem", g_ffn_rem, 1)                              /* remainder rows of GEMM2 on the 4x4x1 MFMA */ \
  B("ffn_split", g_ffn_split, 0)                          /* opt-in bf16x3-split FFN (not the reference's fp32 arithmetic; ffd_ffn_split.hip) */ \
  I("ffn_rows", g_ffn_rows, 1, v >= 0 && v <= 2)          /* large-M FFN: 1 row-owning waves + CU-shared weight ring | 0 k_ffn_ln | 2 at every M (tests) */ \
  I("ffn_rows_nw", g_ffn_rows_nw, 0, v == 0 || v == 4 || v == 8 || v == 12)  /* k_ffn_rows waves per workgroup; 0 heuristic */ \
  I("ffn_rows_cps", g_ffn_rows_cps, 0, v >= 0 && v <= 2)  /* k_ffn_rows 32-unit chunks per ring slot: 0 / 2 two | 1 one */ \
  B("ffn_rows_fuse", g_ffn_rows_fuse, 1)                  /* out-projection + LN1 inside k_ffn_rows (1) | k_linear_res_ln before it (0) */ \
  I("rows_slices", g_rows_slices, 0, v >= -1 && v != 1 && v <= 32)  /* sliced k_ffn_rows at mid-size M: 0 heuristic | -1 off | 2 ... 32 slices forced */ \
  I("rows_slices_fuse", g_rows_slices_fuse, 0, v >= 0 && v <= 2)  /* sliced form: 0 by estimate | 1 out-projection in every unit | 2 k_linear_res_ln once in front */ \
  I("mid_path", g_mid_path, 1, v == 0 || v == 1 || v == 2 || v == 4 || v == 8)  /* 64-row FFN over F slices for mid-size M: 0 off | 1 heuristic | 2 / 4 / 8 forced */ \
  B("small_path", g_small_path, 1)                        /* split out-proj + FFN pair for small M (0: always the larger forms) */ \
  I("small_wgs", g_small_wgs, 0, v >= 0)                  /* most workgroups (row tiles x F splits) of the small-M pair; 0 heuristic */ \
  I("attn_small", g_attn_small, 1, v == 0 || v == 1 || v == 2 || v == 4)  /* small-batch split attention: 0 never | 1 by batch size | 2 / 4 key pieces forced */ \
  I("attn_fused", g_attn_fused, 1, v >= 0 && v <= 1)      /* fused in-projection + attention where a kernel exists | 0 the two-kernel path */ \
  I("attn_hpw", g_attn_hpw, 0, v >= 0 && v <= 2)          /* heads per attention workgroup: 0 heuristic | 1 / 2 */ \
  I("attn_qg", g_attn_qg, 0, v >= 0 && v <= 3)            /* q-tile group size of the attention kernels: 0 heuristic | 1 / 2 / 3 */ \
  B("attn_kvq", g_attn_kvq, 1)                            /* small-batch split attention on the kv | q pack (q projected for own q-tiles only) */ \
  B("attn_static_bound", g_attn_static_bound, 1)          /* fused attention without the per-launch score bound in layers whose weights bound the scores (LayerWeights::attn_bounded) */ \
  B("embed_ldsx", g_embed_ldsx, 1)                        /* embedding: the wave's x rows through LDS (1) | per-lane loads (0) */ \
  I("embed_threads", g_embed_threads, 262144, v >= 256)   /* threads the embed grid aims at (tools/probes/embed_sweep.py: 114 us at 256 k, 118 at 512 k, 137 at 128 k on the config-5 shape) */ \
  I("lstm_wave", g_lstm_wave, 1, v >= 0 && v <= 2)        /* LSTM layers as a wavefront (1, 2 the same) | 0 the per-layer kernels k_linear_rm + k_lstm_layer */ \
  B("lstm_wave_persist", g_lstm_wave_persist, 1)          /* k_lstm_wave workgroups walk their tile's layers (1) | a launch per layer group (0) */ \
  I("lstm_wave_per", g_lstm_wave_per, 0, v >= 0 && v <= 16)  /* at most this many layers in flight (0: as many as the CUs hold) */ \
  I("lstm_wave_chunk", g_lstm_wave_chunk, 0, v >= 0 && !(v > 1 && (v & 1)) && v <= 1024)  /* cell steps per unit of the time-shared wavefront: 0 by the pass count | 1 never | even n forced */ \
  I("lstm_wave_fault", g_lstm_wave_fault, 0, v >= 0)      /* tests: unit (v - 1) of k_lstm_wave never publishes its progress */ \
  I("lstm_wave_spin_ms", g_lstm_wave_spin_ms, 2000, v >= 1 && v <= 20000)  /* time limit of one wait on a progress word */ \
  B("fuse_tail", g_fuse_tail, 1)                          /* unembed inside the SDE-step kernel of ffd_sample_batch */ \
  I("partitions", g_partitions, 1, v >= 0 && v <= 2)      /* the batch as two halves on CU-masked streams: 0 never | 1 where a half fills its CUs | 2 wherever eligible */ \
  I("fail_alloc_after", g_fail_alloc_after, 0, v >= 0)    /* tests: the n-th device allocation from now fails with FFD_ERR_NOMEM (0 off) */

#define FFD_KNOB_DECL(key, var, ...) extern thread_local int var;
FFD_KNOBS(FFD_KNOB_DECL, FFD_KNOB_DECL)
#undef FFD_KNOB_DECL

// ---- LDS-DMA issued by hand + counted waits (k_ffn_rows, k_linear_res_ln) ----
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// One LDS-DMA piece: 64 lanes x 16 B from per-lane global addresses to LDS bytes [lds_byte, lds_byte + 1024).
// Issued from inline asm on purpose: for the builtin form hipcc (ROCm 7.2) puts an s_waitcnt vmcnt(0) in front of the
// next ds_read of the same __shared__ array (it cannot tell the ring's slots apart), which drains the ring every slot.
// The kernels order DMA and reads themselves: counted vmcnt (+ s_barrier where waves share the image).
__device__ __forceinline__ void dma_piece(const float* g, unsigned lds_byte) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_byte), "v"(g)
               : "memory");  // (m0 is a reserved register: hipcc keeps nothing in it across statements)
}
// The same piece from a wave-uniform base (an SGPR pair) + a 32-bit per-lane byte offset (lane x 16 for a contiguous
// piece): the address of each piece is then scalar arithmetic, where the per-lane 64-bit pointer above costs a vector
// 64-bit add per piece (k_ffn_rows: fp32 vector instructions add to its matrix time).
__device__ __forceinline__ void dma_piece_sbase(const float* base, unsigned lane_byte, unsigned lds_byte) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_byte), "v"(lane_byte), "s"(base)
               : "memory");
}
__device__ __forceinline__ unsigned lds_addr(const float* p) {
  return (unsigned)(unsigned long)((const __attribute__((address_space(3))) float*)p);
}


// Padded LDS row stride (in floats) for a (rows x D) fp32 tile whose MFMA
// fragments are read with ds_read_b32 as tile[(l&15)*stride + 4s + (l>>4)]:
// stride/2 odd => the 16 rows x 2 k of each 32-lane half hit 32 distinct banks.
constexpr __host__ __device__ int lds_stride(int D) { return D + ((6 - D % 4) % 4); }

// ---- packed weight layouts -------------------------------------------------
// "dpack": a (N x D) weight (PyTorch (out,in) order) packed as the A operand of
// Y^T = W X^T :  [nt = N/16 tiles][g = ceil(ceil(D/4)/4)][lane 64][j 4]
//   = W[16 nt + (lane & 15)][4 (4 g + j) + (lane >> 4)]   (0 outside N x D)
// so that one coalesced float4 load per lane yields 4 consecutive k-steps.
constexpr __host__ __device__ int dpack_groups(int D) { return cdiv(cdiv(D, 4), 4); }
constexpr __host__ __device__ size_t dpack_floats(int N, int D) {
  return (size_t)cdiv(N, 16) * dpack_groups(D) * 64 * 4;
}
// "w2pack": linear2.weight (D x F) packed as the A operand of Y^T += W2 H^T with
// the GEMM1 accumulator as B:  [fc = F/16][ct = ceil(D/16)][lane 64][r 4]
//   = W2[16 ct + (lane & 15)][16 fc + 4 (lane >> 4) + r]      (0 for c >= D)
constexpr __host__ __device__ size_t w2pack_floats(int D, int F) { return (size_t)(F / 16) * cdiv(D, 16) * 64 * 4; }

// ---- launchers (each returns the hipError_t of the launch) -----------------

struct LayerWeights {
  // raw (device) parameters
  const float *in_w, *in_b, *out_w, *out_b, *w1, *b1, *w2, *b2, *n1w, *n1b, *n2w, *n2b;
  // packed by ffd_finalize_weights (the context owns them); nullptr: no kernel of that form for this shape
  float *in_wp = nullptr, *q_wp = nullptr, *kv_wp = nullptr;  // dpack (3d x d), of its q rows (d x d), of its k | v rows (2d x d)
  float* out_wp = nullptr;  // dpack (d x d)
  float* w1p = nullptr;     // dpack (F x d)
  float* w2p = nullptr;     // w2pack
  float* w2r = nullptr;     // w2rem (remainder rows d % 16 of linear2.weight, 4x4x1 MFMA A-operand order)
  float* ring = nullptr;     // CU-shared weight ring pack of the row-owning FFN (ffd_ffn_rows.hip)
  float* ring_op = nullptr;  // its out-projection slot (fused out-proj + LN1 form)
  float *w1s = nullptr, *w2s = nullptr;  // three-part bf16 packs of the opt-in split FFN (ffd_ffn_split.hip), made on first use
  float *aw_full = nullptr, *aw_q = nullptr;    // per-head packs of the fused in-projection + attention kernel
  float *aw_full2 = nullptr, *aw_q2 = nullptr;  // same, per pair of heads (two-head workgroups)
  float* aw_kvq = nullptr;                      // per head, tile 0 = k | v, tile 1 = q (the split small-batch form)
  // every head's static score bound (ffd_host_attn_score_bound, from the norm2 of the layer in front) is within the
  // attention kernels' threshold: set by ffd_finalize_weights; layer 0 (input: the embedding) never
  bool attn_bounded = false;
};

hipError_t launch_pack_dweight(const float* W, float* Wp, int N, int D, hipStream_t s);
hipError_t launch_pack_w2(const float* W2, float* W2p, int D, int F, hipStream_t s);
// "w2rem": rows c >= 16*(D/16) of linear2.weight (D x F), in groups of 4, as the A operand of
// v_mfma_f32_4x4x1_16b_f32 with a GEMM1 accumulator register r as B (block b = lane>>2 pairs
// A[lane 4b+i] with B[lane 4b+j]):  [fc = F/16][g][lane 64][r 4]
//   = W2[16*(D/16) + 4 g + (lane & 3)][16 fc + 4 (lane >> 4) + r]
constexpr __host__ __device__ int w2rem_groups(int D) { return (D % 16) / 4; }
constexpr __host__ __device__ size_t w2rem_floats(int D, int F) { return (size_t)(F / 16) * (w2rem_groups(D) ? w2rem_groups(D) : 1) * 64 * 4; }
hipError_t launch_pack_w2rem(const float* W2, float* W2r, int D, int F, hipStream_t s);
hipError_t launch_renorm_rows(float* W, int rows, int D, float max_norm, hipStream_t s);

// temb[n][d] = dense(gamma(t_n)) for n timesteps (transformer.py:77-91)
// (ts == nullptr: a single embedding of the immediate t_imm)
hipError_t launch_time_embed(const float* ts, float t_imm, int n, const float* W, const float* dense_w,
                             const float* dense_b, float* temb, int D, hipStream_t s);
// h[b,l,:] = X[b,l,:] We^T + be (+ pos[l,:]) + temb[b * temb_stride + :]   (temb_stride 0: one embedding for the batch)
hipError_t launch_embed(const float* X, const float* We, const float* be, const float* pos, const float* temb,
                        int temb_stride, float* h, int B, int L, int C, int D, hipStream_t s);
// score[b,l,c] = h[b,l,:] . Wu[c,:] + bu[c]
hipError_t launch_unembed(const float* h, const float* Wu, const float* bu, float* score, int M, int C, int D,
                          hipStream_t s);

struct SdeParams {
  int sde;          // 0 VP 1 VE
  float a;          // VP: (float)(-0.5*beta)        VE: unused
  float cs;         // (float)sqrt(beta) | (float)sqrt_derivative
  float dt, sqdt;   // step_size, sqrtf(step_size)
};
SdeParams sde_params(int sde, double a, double b, double t, float step_size);  // the step at time t (sde.py:143-147, 212-213)
hipError_t launch_sde_step(float* x, const float* score, const float* z, const float* G, SdeParams p, uint64_t seed,
                           uint64_t elem_offset, uint32_t step, int B, int L, int C, hipStream_t s);
// the two fused: x <- step(x, unembed(h)); the score stays in registers.  Needs unembed_sde_supported(C, D).
bool unembed_sde_supported(int C, int D);
hipError_t launch_unembed_sde(const float* h, const float* Wu, const float* bu, float* x, const float* z, const float* G,
                              SdeParams p, uint64_t seed, uint64_t elem_offset, uint32_t step, int B, int L, int C,
                              int D, hipStream_t s);
// The probability-flow ODE tails (ffd_elem.hip).  p = sde_params at the time of the score evaluation (sqdt unused).
//   ODE_EULER    x <- x - d(x, score) dt                                       (xp, d1 unused)
//   ODE_PREDICT  d1 <- d(x, score);  xp <- x - d1 dt                           (x is not modified)
//   ODE_CORRECT  x <- x - (1/2 (d1 + d(xp, score))) dt, score = the score at xp, p at the interval's end
// x, xp and d1 are distinct (B, L, C) buffers.
enum OdeTail { ODE_EULER = 0, ODE_PREDICT = 1, ODE_CORRECT = 2 };
hipError_t launch_ode_step(int tail, float* x, const float* score, float* xp, float* d1, const float* G, SdeParams p,
                           int B, int L, int C, hipStream_t s);
// ... with the unembedding inside (the score stays in registers).  Needs unembed_sde_supported(C, D).
hipError_t launch_unembed_ode(int tail, const float* h, const float* Wu, const float* bu, float* x, float* xp, float* d1,
                              const float* G, SdeParams p, int B, int L, int C, int D, hipStream_t s);
// The linear multistep tail (ffd_elem.hip; include/ffd.h ffd_ode_multistep_step): AB2 and DPM-Solver++ 2M are this one
// operation with the five coefficients multistep_coef computes in double and multistep_params rounds once,
//   q = (qa x) + (qb ((G_l G_l) score));  x <- x + ((cxm1 x) + (cn q) [+ (cp hist)]);  hist <- q.
// have_prev == 0 (a trajectory's first interval): hist is written only.  x and hist are distinct (B, L, C) buffers.
struct MultistepParams { float qa, qb, cxm1, cn, cp; };
int multistep_coef(int sde, double a, double b, int solver, double t_prev, double t, double t_next, double step_size,
                   int have_prev, double* coef_out);  // FFD_OK | FFD_ERR_INVALID
MultistepParams multistep_params(const double* coef);
hipError_t launch_multistep_step(float* x, const float* score, float* hist, const float* G, MultistepParams p,
                                 int have_prev, int B, int L, int C, hipStream_t s);
// ... with the unembedding inside (the score stays in registers).  Needs unembed_sde_supported(C, D).
hipError_t launch_unembed_multistep(const float* h, const float* Wu, const float* bu, float* x, float* hist, const float* G,
                                    MultistepParams p, int have_prev, int B, int L, int C, int D, hipStream_t s);

// The Langevin corrector (ffd_langevin.hip; include/ffd.h ffd_langevin_step): row squares, step size, update, four
// launches with the batch norm and three with the sample norm.  alpha = langevin_alpha at the evaluation's time;
// work = langevin_work_bytes(B, L) bytes, 16-byte aligned; eps_out nullptr or (B).
size_t langevin_work_bytes(int B, int L);
double langevin_alpha(int sde, double a, double b, double t, float step_size);
hipError_t launch_langevin(float* x, const float* score, const float* z, const float* G, double alpha, double snr,
                           int norm, uint64_t seed, uint64_t elem_offset, uint32_t tag, int B, int L, int C,
                           float* eps_out, void* work, hipStream_t s);

// Log-likelihoods through the probability-flow ODE (ffd_loglik.hip; include/ffd.h ffd_loglik_tail).  One divergence
// evaluation: launch_loglik_perturb writes the stacked batch of (1 + 2 k) B rows, the caller evaluates the score there,
// launch_loglik_tail reduces the probes' terms per sample, updates the state from block 0's score and accumulates
// delta (LL_EULER, LL_CORRECT) or keeps v1 (LL_PREDICT).  Probes: injected (k, B, L, C), or Rademacher draws under tags
// tag0 + m at global element elem_offset + i.  dt: the interval's width in double (the state moves by (float)dt).
enum LoglikStage { LL_EULER = 0, LL_PREDICT = 1, LL_CORRECT = 2 };  // = FFD_LOGLIK_*
struct LoglikProbes {
  const float* inject;
  uint64_t seed, elem_offset;
  uint32_t tag0;
  int k;
};
double loglik_sigma(int sde, double a, double b, double t);  // the marginal's standard deviation without G, in double
bool loglik_shape_supported(int n_probes, int B, int L, int C);  // (1 + 2 k) B L C < 2^31
hipError_t launch_loglik_perturb(const float* x, float* stack, const float* G, float h, LoglikProbes pr, int B, int L, int C,
                                 hipStream_t s);
hipError_t launch_loglik_tail(int stage, int sde, double a, double b, double t, double dt, float h, float* x, float* xp,
                              float* d1, const float* score, const float* G, LoglikProbes pr, double* delta, double* v1,
                              double* v_out, int B, int L, int C, hipStream_t s);
hipError_t launch_prior_logp(const float* x, const float* G, float scale, double* out, int B, int L, int C, hipStream_t s);

// Conditional sampling by replacement (include/ffd.h ffd_cond_project).  cond_coeffs: the marginal's (mc, sigma) at t in
// double, rounded once (noiseless: 1, 0).  launch_cond_project: the frequency-domain projection (ffd_fft.hip), one launch;
// hipErrorInvalidValue for a length outside cond_len_supported.  launch_cond_time: the pointwise one (ffd_elem.hip).
void cond_coeffs(int sde, double a, double b, double t, int noiseless, float* mc, float* sigma);
bool cond_len_supported(int L);
hipError_t launch_cond_project(float* x, const float* obs, const float* mask, const float* std, const float* G, float mc,
                               float sigma, int noiseless, const float* z, uint64_t seed, uint64_t elem_offset, uint32_t tag,
                               int obs_batch, int B, int L, int C, hipStream_t s);
hipError_t launch_cond_time(float* x, const float* obs, const float* mask, const float* G, float mc, float sigma,
                            int noiseless, const float* z, uint64_t seed, uint64_t elem_offset, uint32_t tag, int obs_batch,
                            int B, int L, int C, hipStream_t s);
// Reconstruction guidance (include/ffd.h ffd_guide_seed; ffd_guide.hip, the frequency-domain seed next to
// k_cond_project in ffd_fft.hip).  guide_coef: (alpha, sigma^2, lambda) at t in double, FFD_ERR_INVALID as
// ffd_host_guide_coef (the SDE kind is the caller's to check).
struct GuideArgs {
  const float *x, *score, *obs, *mask, *std, *G;
  float *u, *v, *x0hat;  // x0hat: nullptr or the denoised estimate
  double* loss;          // nullptr or B doubles
  float alpha, sigma2;
  int obs_batch;
};
// c = sigma^2 (G_l G_l) of packed row r and x0hat = (x + c s) / alpha, every operation its own fp32 rounding
__device__ __forceinline__ float guide_c(const GuideArgs& a, int r) {
  const float g = a.G[r];
  return __fmul_rn(a.sigma2, __fmul_rn(g, g));
}
__device__ __forceinline__ float guide_x0hat(const GuideArgs& a, size_t ix, float c) {
  return __fdiv_rn(__fadd_rn(a.x[ix], __fmul_rn(c, a.score[ix])), a.alpha);
}
int guide_coef(int sde, double a, double b, double t, double scale, double obs_var, double rho, double coef[3]);
hipError_t launch_guide_seed_time(const GuideArgs& a, int B, int L, int C, hipStream_t s);
hipError_t launch_guide_seed_freq(const GuideArgs& a, int B, int L, int C, hipStream_t s);  // hipErrorInvalidValue: length
hipError_t launch_guide_combine(const float* score, const float* u, const float* jtv, float alpha, float coef, float* out,
                                size_t n, hipStream_t s);
// the descriptor a training object was created with (ffd_train.hip; ffd_sample_batch_guided compares it with the context's)
const ffd_model_desc& train_desc(const ffd_train* tr);
// The forward transition s -> t of the SDE (include/ffd.h ffd_forward_transition; ffd_elem.hip).  transition_coef: (a, sg)
// in double, FFD_ERR_INVALID / FFD_ERR_UNSUPPORTED as ffd_host_transition_coef.  The launch is skipped for (1, 0).
int transition_coef(int sde, double a, double b, double s, double t, double* coef);
hipError_t launch_forward_transition(float* x, const float* G, float a, float sg, const float* z, uint64_t seed,
                                     uint64_t elem_offset, uint32_t tag, int B, int L, int C, hipStream_t s);

// Denoising score-matching loss (ffd_loss.hip; losses.py:54-125).  Sample b of the call is global sample
// sample_offset + b: with z == nullptr both kernels take the draw of global element g from slot g & 3 of Philox block
// g >> 2 under SM_TAG_NOISE, so the loss regenerates what the perturbation drew.
constexpr uint32_t SM_TAG_NOISE = 0xFFFFFFFEu, SM_TAG_TIMES = 0xFFFFFFFDu;  // (0xFFFFFFFF: the prior; below 2^31: step indices)
constexpr uint32_t SM_TAG_CLASS_DROP = 0xFFFFFFFCu;  // the training-time label dropout (loglik's probes end at 0xFFFFFFF0)
// Class conditioning and classifier-free guidance (ffd_class.hip; include/ffd.h ffd_class_temb ...).
// launch_class_temb: the (B | 2 B, d) embedding rows; xs != nullptr: the same launch also writes x (nx floats) to both
// halves of xs (the stacked batch).  labels nullptr: every row null.
hipError_t launch_class_temb(const float* temb, int temb_stride, const float* table, int n_classes, const int32_t* labels,
                             int B, int d, int stack, float* out, const float* x, float* xs, size_t nx, hipStream_t s);
hipError_t launch_cfg_combine(float* c, const float* u, float g, size_t n, hipStream_t s);
hipError_t launch_class_drop(const int32_t* labels, int n_classes, const int64_t* index, int B, float p_uncond, uint64_t seed,
                             uint64_t sample_offset, int32_t* out, hipStream_t s);
hipError_t launch_class_table_grad(const float* dtemb, const int32_t* eff_labels, int n_classes, int B, int d, float* dtable,
                                   hipStream_t s);
// x_noisy[b,l,c] = mean_coeff[b] * x0[b,l,c] + (sigma[b] * G[l]) * z[b,l,c]
hipError_t launch_sm_perturb(const float* x0, float* x_noisy, const float* mean_coeff, const float* sigma, const float* G,
                             const float* z, uint64_t seed, uint64_t sample_offset, int B, int L, int C, hipStream_t s);
// out[b] = the reduced, weighted squared error of sample b (B doubles)
hipError_t launch_sm_loss(const float* score, const float* sigma, const float* G, const float* z, uint64_t seed,
                          uint64_t sample_offset, int likelihood_weighting, int reduce_mean, double* out, int B, int L,
                          int C, hipStream_t s);

// Y[M x N] (row stride ldy) = X[M x D] Wp^T + b ; Wp is dpack of the N x D weight.
hipError_t launch_linear(const float* X, const float* Wp, const float* bias, float* Y, int M, int N, int D, int ldy,
                         hipStream_t s);
// Y[M x D] = LayerNorm(R + X Wp^T + b) * g + beta    (out-proj + residual + LN1)
hipError_t launch_linear_res_ln(const float* X, const float* Wp, const float* bias, const float* R, const float* g,
                                const float* beta, float* Y, int M, int D, hipStream_t s);
// Fused FFN: Y = LN2(X + W2 relu(W1 X + b1) + b2) in 16 mb-row tiles (k_ffn_ln); rem: the instance with GEMM2's remainder
// rows on the 4x4x1 MFMA (only where ffn_rem_rows); persist (mb = 4): 0 a workgroup per tile, n: a grid of n x the resident ones
// stamp != nullptr (diagnostics): per-workgroup (shader-clock, 100 MHz real-time) deltas around the main loop
bool ffn_rem_rows(int D, int mb);
hipError_t launch_ffn_ln(const float* X, const LayerWeights& w, float* Y, int M, int D, int F, int mb, bool rem, int persist,
                         hipStream_t s, unsigned long long* stamp = nullptr);
// 16-row tiles per CU between 1.4 and 3: k_ffn_ln at 32 / 48 rows per workgroup (one tile per CU); 0 = not this form
int ffn_height_plan(int M, int D, int F);
// ... as ONE launch (mb = 1 / 2 / 3), out-projection + LN1 inside; Y may be Rres
hipError_t launch_oproj_ffn_ln(const float* attn, const float* Rres, const LayerWeights& w, float* Y, int M, int D, int F,
                               int mb, bool rem, hipStream_t s);
// Row-owning FFN with a CU-shared LDS weight ring (ffd_ffn_rows.hip): the large-M form
bool ffn_rows_supported(int D, int F);
bool ffn_rows_selected(int M, int D, int F);
size_t ffn_ring_floats(int D, int F);
hipError_t launch_pack_ffn_ring(const float* W1, const float* b1, const float* W2, float* out, int D, int F, hipStream_t s);
// One k_ffn_rows launch as the plan says: nw waves per workgroup, cps 32-unit chunks per ring slot
struct RowsGrid {
  int grid, ntiles;  // workgroups of the launch; row tiles of 32 nw rows (grid == ntiles: the one-workgroup-per-tile instance)
};
struct RowsArgs {
  const float *X, *Rin;  // fused: attention output + layer input; else the FFN input (Rin unused)
  const LayerWeights* w;
  float* Y;  // fused: must not alias X / Rin (rows are read and written by different waves); sliced: the partial rows
  int M, D, F;
  int nw, cps;
  bool fused;  // out-proj + LN1 + FFN + LN2 in one launch: Y = LN2(x1 + FFN(x1)), x1 = LN1(Rin + Wo X + bo)
  int nslice;  // >= 2: the sliced form of mid-size M, tiles x nslice units (Y = [nslice][M][D]); 0: whole rows
  unsigned long long* stamp;
  RowsGrid* grid_only = nullptr;  // the launcher reports the grid it would launch here and launches nothing (ffd_partition_plan)
};
int rows_waves(int M);  // waves per workgroup of the unsliced forms
hipError_t launch_ffn_rows(const RowsArgs& a, hipStream_t s);
bool ffn_rows_fused_selected(int M, int D, int F);
size_t ffn_ring_oproj_floats(int D);
hipError_t launch_pack_oproj_ring(const float* Wo, float* out, int D, hipStream_t s);
// mid-size M: the kernel over tiles x slices of the hidden dimension, then Y = LN2(the partial rows P added in slice order)
bool rows_slice_plan(int M, int D, int F, int* nw_out, int* nslice_out, int* unfused_out);
size_t rows_slice_floats(int M, int D, int nslice);
hipError_t launch_rows_reduce_ln(const float* P, const LayerWeights& w, float* Y, int M, int D, int nslice, hipStream_t s);
// Small M (the reference harness's batch 1): out-proj + LN1 + FFN + LN2 as two launches with F split over NS
// workgroups per 16-row tile (ffd_small.hip).  small_path_splits returns 0 where this form does not apply.
int small_path_splits(int M, int D, int F);
size_t small_path_partial_floats(int M, int D, int NS);
hipError_t launch_oproj_ffn_small(const float* attn, const float* xres, const LayerWeights& w, float* x1, float* P,
                                  float* Y, int M, int D, int F, int NS, hipStream_t s);
// Mid-size M: the 64-row FFN main loop over F slices + the same reduce (ffd_small.hip); 0 = not this form
int mid_path_splits(int M, int D, int F);
hipError_t launch_ffn_mid(const float* x1, const LayerWeights& w, float* P, float* Y, int M, int D, int F, int NS, hipStream_t s);
bool ffn_split_supported(int D, int F);
size_t w1split_bytes(int D, int F);
size_t w2split_bytes(int D, int F);
hipError_t launch_pack_ffn_split(const float* W1, const float* W2, void* w1s, void* w2s, int D, int F, hipStream_t s);
hipError_t launch_ffn_ln_split(const float* X, const LayerWeights& w, float* Y, int M, int D, int F, hipStream_t s,
                               unsigned long long* stamp = nullptr);
// fused in-projection + attention (ffd_qkvattn.hip)
// scores (log2 domain) may sit this far from the softmax reference before it is refreshed; a head whose |q| |k| stays
// within it needs no running maximum (head_norms per launch, or LayerWeights::attn_bounded from the weights)
constexpr float ATTN_SCORE_T = 64.0f;
float attn_q_scale(int hd);  // log2(e) / sqrt(hd), as launch_pack_attn folds it into the q rows of the packs
size_t attn_pack_floats(int D, int H, int hpw, int q_only);  // q_only = pack mode: 0 q | k | v, 1 q only, 2 tile 0 = k | v, tile 1 = q
bool attn_kvq_supported(int hd);                              // head dims with a mode-2 pack (the split small-batch form's)
hipError_t launch_pack_attn(const float* in_w, const float* in_b, float* pack, int D, int H, int hpw, int q_only,
                            hipStream_t s);
bool qkv_attention_supported(int D, int hd);
int qkv_attention_hpw(int D, int hd, int L);
int qkv_attention_small_split(int B, int H, int L);
int attn_qg(int QT, int hd, bool fused);  // q-tiles per wave at QT q-tiles: of k_qkv_attention (fused), else of k_attention_mfma
// workgroups of launch_ffn_ln's grid (the launcher's own rule); *ntiles_out: the 16 mb-row tiles
int ffn_ln_grid(int M, int mb, int persist, int* ntiles_out);
int num_cus();  // compute units the calling thread's launches may count on: g_cu_budget, else the current device's (256 on MI355X); ffd_ffn.hip
// > 0 while the calling thread enqueues one CU partition's half of a batch (ffd_api.hip run_partitioned): the planner, the
// form pickers and the grids then size themselves for that many CUs
extern thread_local int g_cu_budget;
struct AttnArgs {
  const float *x, *pack;    // the layer's input rows; the in-projection pack that (hpw, q_only) name
  const float *kt, *vt;     // the layer's K/V tables to read (cached modes), else nullptr
  float *kt_out, *vt_out;   // where batch element 0's recomputed rows go (MIXED), else nullptr
  float* out;               // (M x d) row-major
  int B, L, n_own;          // tokens >= n_own take K/V from the tables
  unsigned long long* stamp;
  bool static_bound = false;  // the layer's scores are bounded by its weights: the instance without head_norms (kt == nullptr only)
};
// kspl > 0: the small-batch split form with that many key pieces per q-tile (hpw 1; no stamped twin); else qg q-tiles per
// wave (hpw 2: per wave pair)
hipError_t launch_qkv_attention(const AttnArgs& a, int D, int hd, int hpw, int q_only, int kspl, int qg, hipStream_t s);

// Head-major projection: columns [r*d, (r+1)*d) of Y = X Wp^T + b go to region out[r]
// laid out (B, H, L, hd) -- each (sample, head) slice contiguous, the layout of the K/V tables.
hipError_t launch_linear_hm(const float* X, const float* Wp, const float* bias, float* out0, float* out1, float* out2,
                            int M, int nreg, int D, int L, int H, int hd, hipStream_t s);
// attention over head-major q, k, v (B,H,L,hd); tokens >= n_own take K/V from the
// (H,L,hd) tables kt/vt instead of the sample's own rows. out: (M x d) row-major.  qg: q-tiles per wave (1 / 2 / 3)
hipError_t launch_attention(const float* q, const float* k, const float* v, const float* kt, const float* vt,
                            float* out, int B, int L, int H, int hd, int n_own, int qg, hipStream_t s);
// table[h][l][:] (l < n) <- sample 0's head-major K/V rows
hipError_t launch_kv_store(const float* k, const float* v, float* kt, float* vt, int L, int H, int hd, int n,
                           hipStream_t s);
// crf[l][:] <- h[l][:] for sample 0 is a plain D2D copy (done with hipMemcpyAsync)

hipError_t launch_lstm_layer(float* x, const float* gx, const float* whh, int B, int L, int D, hipStream_t s);
// batches below that kernel's crossover: all layers as a wavefront of (16-sample tile, layer) workgroups, in place on x;
// prog: >= 16 + 16 * ceil(B / 16) ints of device scratch (abort word + progress words, cleared by the launcher);
// err: host-visible word that receives 1 + (unit index) when a wait on a progress word runs out of time
int lstm_wave_max_batch(int L, int D);  // samples one k_lstm_wave launch takes (a 16-sample tile per CU, rows < 2^31 bytes); larger batches go in sub-batches
hipError_t launch_lstm_wave(float* x, const float* const* wih_pk, const float* const* whh_pk, const float* const* bias_pk, int NL,
                            int B, int L, int D, int* prog, float* state, int* err, hipStream_t s,
                            unsigned long long* trace = nullptr);  // trace: 4 u64 per unit (ffd_lstm_trace), diagnostics
size_t lstm_wave_state_floats(int B, int D, int NL);
// launch_lstm_wave takes the weights in k_lstm_wave's fragment order (one pack per role and layer + the summed bias)
size_t lstm_wave_wpack_floats(int D);
size_t lstm_wave_bpack_floats(int D);
hipError_t launch_pack_lstm_wave(const float* wih, const float* whh, const float* bsum, float* ih_out, float* hh_out,
                                 float* b_out, int D, hipStream_t s);

hipError_t launch_dense(const float* X, const float* W, const float* b, const float* b2, const float* R, float* Y,
                        int M, int N, int K, int relu, hipStream_t s);
// ---- lengths of the LDS-resident transforms (ffd_fft.hip): the one statement of the limits, repeated in ffd.h ----
// A workgroup keeps the length-L twiddle table and two complex slabs of CG >= 1 channels in at most 160 KiB of LDS:
// (L + L CG) float2 for a power of two (a half-length complex transform), (L + 2 L CG) float2 for any other length.
// So every power of two up to FFT_MAX_LEN = 8192 is taken, and any other length up to FFT_MAX_MIXED_LEN = 6826
// (3 * 6826 float2 = 163 824 B; 6827 needs 163 848 B).  FreSca and the decomposition stop at FFT_MAX_FILTER_LEN.
// Every entry point that transforms asks fft_len_supported before its first device call.
constexpr int FFT_MAX_LEN = 8192, FFT_MAX_FILTER_LEN = 4096;
constexpr size_t FFT_LDS_CAP = 160 * 1024;
constexpr bool fft_len_is_pow2(int L) { return L >= 2 && (L & (L - 1)) == 0; }
constexpr size_t fft_lds_bytes(int L, int CG) {  // twiddles + two slabs of CG channels
  return (size_t)L * (fft_len_is_pow2(L) ? 1 + (size_t)CG : 1 + 2 * (size_t)CG) * 8;
}
constexpr bool fft_len_supported(int L, int max_len = FFT_MAX_LEN) {
  return L >= 1 && L <= max_len && fft_lds_bytes(L, 1) <= FFT_LDS_CAP;
}
constexpr int fft_max_mixed_len() {  // the longest supported length that is not a power of two
  int L = FFT_MAX_LEN;
  while (fft_len_is_pow2(L) || !fft_len_supported(L)) --L;
  return L;
}
constexpr int FFT_MAX_MIXED_LEN = fft_max_mixed_len();
static_assert(FFT_MAX_MIXED_LEN == 6826, "ffd.h states this length");
// FreSca spectral scaling of a (B,L,C) score; work: B*(L/2+1) + 1 floats; strategy 0 spatial, 1 energy
hipError_t launch_fresca(const float* in, float* out, float* work, int B, int L, int C, float low, float high,
                         double cutoff_ratio, int strategy, hipStream_t s);

// ---- the closed-form Gaussian-mixture score (ffd_mixture.hip; include/ffd.h ffd_mixture_score) ----
// Tiling: 16 rows x 16 components per step, slices of 512 components per workgroup column, L * C up to 1024.  The
// tiling depends on K and L * C alone (never on B): a row's bits do not depend on the batch it is evaluated in.
constexpr int MIX_ROW_TILE = 16, MIX_COMP_TILE = 16, MIX_SLICE = 512, MIX_MAX_DIM = 1024;
bool mixture_shape_supported(int B, int K, int L, int C);
size_t mixture_work_floats(int B, int K, int L, int C);  // 0 for a shape the launch refuses
// t: device, row r reads t[r * t_stride] (t_stride 0 | 1); var nullptr: v = 0; work: mixture_work_floats floats.
// hipErrorInvalidValue for an unsupported shape.
hipError_t launch_mixture_score(int sde, double sa, double sb, const float* x, const float* t, int t_stride,
                                const float* means, const float* logw, const float* var, const float* G, float* out, int B,
                                int K, int L, int C, float* work, hipStream_t s);
// out = J^T v, J = d score / d x (symmetric), v (B, L, C); work: mixture_vjp_work_floats floats; out may be v or x.
size_t mixture_vjp_work_floats(int B, int K, int L, int C);  // 0 for a shape the launch refuses
hipError_t launch_mixture_score_vjp(int sde, double sa, double sb, const float* x, const float* t, int t_stride,
                                    const float* means, const float* logw, const float* var, const float* G, const float* v,
                                    float* out, int B, int K, int L, int C, float* work, hipStream_t s);
// out[i] = ts[i] (ts == nullptr: the immediate t_imm), n floats: the mixture kind's "time embedding" is the time itself
hipError_t launch_mixture_times(const float* ts, float t_imm, int n, float* out, hipStream_t s);
// host: FFD_OK | FFD_ERR_INVALID (non-finite mean, negative / non-finite variance, NaN / +inf log-weight, all -inf) |
// FFD_ERR_UNSUPPORTED (L * C over MIX_MAX_DIM); *why (may be nullptr) names the reason (static string)
int mixture_check(const float* means, const float* logw, const float* var, int K, int L, int C, const char** why);

// ---- pieces of the sample metrics (ffd_metrics.hip) that the ensemble scores (ffd_ensemble.hip) run as they are ----
// P (Kb, N) = columns [f0, f0 + Kb) of X (N, D): the tiled transpose through LDS; Kb <= 32768 * 32
hipError_t launch_w2_columns(const float* X, float* P, int N, int D, int f0, int Kb, hipStream_t s);
// Sort the Kb <= 65535 rows of `rows` (Kb, N) ascending in place (8192-key chunks, then merge passes; -0.0 before +0.0);
// `scratch` holds Kb * N more words
hipError_t launch_w2_sort(float* rows, float* scratch, int N, int Kb, hipStream_t s);

// ---- the kernels of one transformer layer / of the LSTM stack at a batch (ffd_api.hip) --------------------------
// plan_layer is the one place that orders the forms and picks their instances; each heuristic above answers for its own
// form only, and the launchers map the plan to a kernel without reading a knob.
enum CacheMode { CACHE_STD, CACHE_FULL, CACHE_PURE, CACHE_MIXED };  // cached_transformer.py:139-220
CacheMode cache_mode(int n_rec, int L);  // n_rec < 0: no cache
enum AttnForm { ATTN_FUSED, ATTN_TWO_KERNEL };  // k_qkv_attention | k_linear_hm + k_attention_mfma (+ k_kv_store)
// FFD_K_FFN forms: the first four take the out-projection + LN1 in, the other five run behind k_linear_res_ln
enum FfnForm { FFN_LN_OPROJ, FFN_SMALL, FFN_ROWS_SLICED_OPROJ, FFN_ROWS_OPROJ, FFN_ROWS_SLICED, FFN_MID, FFN_SPLIT, FFN_ROWS,
               FFN_LN };
struct PackSet {  // the per-layer packs ffd_finalize_weights made for this shape
  bool aw_full, aw_full2, aw_kvq;  // fused attention: per head, per head pair, kv | q
  bool ring;                       // k_ffn_rows weight ring + its out-projection slot
};
struct LayerPlan {
  AttnForm attn;
  int hpw;     // heads per workgroup
  int q_only;  // 0 q | k | v pack, 1 q only (pure cache hit), 2 kv | q pack
  int kspl;    // key pieces of the small-batch split form, 0 = one workgroup per head (pair)
  int qg;      // q-tiles per wave (per wave pair at hpw 2; 1 in the split form)
  bool attn_static;  // fused kernels: layers with LayerWeights::attn_bounded run the instances without head_norms
  FfnForm ffn;
  int mb;              // FFN_LN_OPROJ / FFN_LN: 16-row tiles per workgroup
  bool rem;            //   GEMM2's remainder rows on the 4x4x1 MFMA
  int persist;         //   FFN_LN at mb 4: 0 a workgroup per tile, n a grid of n x the resident workgroups
  int ns;              // FFN_SMALL: F splits
  int nw, cps;         // FFN_ROWS*: waves per workgroup, 32-unit chunks per ring slot
  int nslice;          // FFN_ROWS_SLICED*: slices
  int nm;              // FFN_MID: F slices
  bool oproj_separate;  // k_linear_res_ln (attn, residual -> x1 in the other hidden buffer) runs in front
  bool swap;            // the output lands in the other hidden buffer
  size_t part_floats;   // partial-buffer floats the form needs
};
LayerPlan plan_layer(const ffd_model_desc& m, int B, CacheMode mode, const PackSet& packs);
struct LstmPlan {
  bool wave;  // k_lstm_wave (all layers) in sub-batches of Bw samples | k_linear_rm + k_lstm_layer per layer
  int Bw;
};
LstmPlan plan_lstm(const ffd_model_desc& m, int B);

}  // namespace ffd
