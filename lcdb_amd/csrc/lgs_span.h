// lgs_span.h -- the byte copy the entry kernels share (lgs_scan.hip's and
// lgs_merge.hip's emits): a group of 16 lanes moves one span.
#pragma once

#include "lgs_device.h"

namespace lgs {

constexpr uint32_t kSpanLanes = 16;   // lanes per entry in the copy

typedef u32x4 u32x4_a1 __attribute__((aligned(1)));

// len bytes from s to d by the kSpanLanes lanes of a group (lane gl): the whole
// 16-byte destination granules with one unaligned load and one aligned store
// each, and the ragged ends (under 16 bytes each) a byte per lane, so a short
// span is one store instruction of the group instead of a loop of one lane
// (keys are mostly short spans: a delta, and a prefix piece per link).  Reads
// and writes stay inside [s, s + len) and [d, d + len).
__device__ __forceinline__ void copy_span(gptr<const uint8_t> s, gptr<uint8_t> d, uint32_t len,
                                          uint32_t gl) {
  const uint32_t lead = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  const uint32_t head = lead < len ? lead : len;
  if (gl < head) d[gl] = s[gl];
  const uint32_t mid = (len - head) & ~15u, body = head + mid;
  for (uint32_t k = head + 16u * gl; k < body; k += 16u * kSpanLanes)
    *(gptr<u32x4>)(d + k) = *(gptr<const u32x4_a1>)(s + k);
  if (gl < len - body) d[body + gl] = s[body + gl];
}

}  // namespace lgs
