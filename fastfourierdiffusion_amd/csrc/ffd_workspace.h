// Host-only helpers of the entry points that take a caller's workspace: the round-up, a carver that lays pieces out at
// 16-byte offsets, the alignment-and-size test of the workspace, and the one check that no written region meets another
// region.  Nothing of HIP is needed here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace ffd {

static inline size_t nn_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Lays a workspace out piece by piece: take(bytes) is the piece's offset, every piece starts on a multiple of 16.
struct Carver {
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t at = total;
    total += nn_up(bytes, 16);
    return at;
  }
};

static inline bool work_ok(const void* work, size_t work_bytes, size_t need) {
  return ((uintptr_t)work & 15) == 0 && work_bytes >= need;
}

struct Region {
  const void* ptr;  // nullptr: an optional region left out, it meets nothing
  size_t bytes;
};
static inline bool regions_meet(const Region& a, const Region& b) {
  const uintptr_t a0 = (uintptr_t)a.ptr, b0 = (uintptr_t)b.ptr;
  return a.ptr && b.ptr && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
// true where a written region (the workspace is one) meets another written region or a read one; read regions may meet
static inline bool regions_clash(std::initializer_list<Region> written, std::initializer_list<Region> read) {
  for (const Region* w = written.begin(); w != written.end(); ++w) {
    for (const Region* o = w + 1; o != written.end(); ++o)
      if (regions_meet(*w, *o)) return true;
    for (const Region& r : read)
      if (regions_meet(*w, r)) return true;
  }
  return false;
}

}  // namespace ffd
