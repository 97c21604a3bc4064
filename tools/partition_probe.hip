// Helper library of tools/partition_probe.py: CU-masked streams, a "where did I run" kernel and a timed delay kernel.
//   hipcc -O2 -fPIC -shared --offload-arch=gfx950 -o tools/libpartition_probe.so tools/partition_probe.hip
// Every entry returns the hipError_t of the first failing runtime call (0 = success).  Not on the product path.
#include <hip/hip_runtime.h>

#include <cstdint>

#define PP_TRY(x)                      \
  do {                                 \
    const hipError_t e_ = (x);         \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

// One record per workgroup: the CU it ran on as __smid() packs it (xcc | se | cu).  The workgroup then keeps its CU for
// hold_ticks of the constant-rate wall clock (an iteration cap bounds the loop), so that a grid larger than the chip
// reaches every CU the stream's mask enables.
__global__ void k_pp_where(unsigned* out, unsigned long long hold_ticks) {
  const unsigned long long t0 = wall_clock64();
  const unsigned id = __smid();
  for (int i = 0; i < (1 << 16) && wall_clock64() - t0 < hold_ticks; ++i) __builtin_amdgcn_s_sleep(16);
  if (threadIdx.x == 0) out[blockIdx.x] = id;
}

// One wave that ends after `ticks` of the wall clock (or after the iteration cap): a start offset for what follows on
// its stream.  It waits on nothing but the clock.
__global__ void k_pp_delay(unsigned long long ticks, unsigned long long* sink) {
  const unsigned long long t0 = wall_clock64();
  unsigned long long t = t0;
  for (int i = 0; i < (1 << 22) && t - t0 < ticks; ++i) {
    __builtin_amdgcn_s_sleep(32);
    t = wall_clock64();
  }
  if (sink && threadIdx.x == 0) *sink = t - t0;
}

extern "C" {

// words > 0: a stream confined to the CUs whose bits are set in mask[0 .. words); words == 0: a plain non-blocking stream
int pp_stream_create(void** out, const uint32_t* mask, int words) {
  hipStream_t s = nullptr;
  if (words > 0)
    PP_TRY(hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask));
  else
    PP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *out = s;
  return 0;
}
int pp_stream_destroy(void* s) { return (int)hipStreamDestroy((hipStream_t)s); }
int pp_stream_sync(void* s) { return (int)hipStreamSynchronize((hipStream_t)s); }

int pp_event_create(void** out) {
  hipEvent_t e = nullptr;
  PP_TRY(hipEventCreate(&e));
  *out = e;
  return 0;
}
int pp_event_destroy(void* e) { return (int)hipEventDestroy((hipEvent_t)e); }
int pp_event_record(void* e, void* s) { return (int)hipEventRecord((hipEvent_t)e, (hipStream_t)s); }
int pp_stream_wait(void* s, void* e) { return (int)hipStreamWaitEvent((hipStream_t)s, (hipEvent_t)e, 0); }
int pp_event_ms(void* e0, void* e1, float* ms) { return (int)hipEventElapsedTime(ms, (hipEvent_t)e0, (hipEvent_t)e1); }

// kHz of wall_clock64 on the current device
int pp_wall_clock_khz(int* khz) {
  int dev = 0;
  PP_TRY(hipGetDevice(&dev));
  return (int)hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, dev);
}
// widths of the se and cu fields of __smid() (the xcc id sits above them)
void pp_smid_bits(int* se_bits, int* cu_bits) {
  *se_bits = HW_ID_SE_ID_SIZE;
  *cu_bits = HW_ID_CU_ID_SIZE;
}

// n_wgs workgroups of `threads` threads on `stream`, each holding its CU for hold_ticks; host_out[n_wgs] receives their
// __smid() values.  Synchronises the stream.
int pp_where(void* stream, int n_wgs, int threads, unsigned long long hold_ticks, unsigned* host_out) {
  if (n_wgs < 1 || n_wgs > (1 << 20) || threads < 64 || threads > 1024 || !host_out) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  unsigned* d = nullptr;
  PP_TRY(hipMalloc((void**)&d, sizeof(unsigned) * (size_t)n_wgs));
  hipLaunchKernelGGL(k_pp_where, dim3(n_wgs), dim3(threads), 0, s, d, hold_ticks);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host_out, d, sizeof(unsigned) * (size_t)n_wgs, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  return (int)e;
}

int pp_delay(void* stream, unsigned long long ticks) {
  hipLaunchKernelGGL(k_pp_delay, dim3(1), dim3(64), 0, (hipStream_t)stream, ticks, (unsigned long long*)nullptr);
  return (int)hipGetLastError();
}

}  // extern "C"
