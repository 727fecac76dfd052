// lgs_host.h -- what the host runtime's two translation units share:
// lgs_api.cpp (the runtime core, the drop-in, the service and the codec and
// bloom batch API) and lgs_table_api.cpp (the SSTable runtime).
//
// Everything with state (the error buffer, the context pools, the staging
// threads, the options) is defined once, in lgs_api.cpp, and only declared
// here; what is defined here is stateless and inline.  None of these names
// leaves the library (exports.map).
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <vector>

#include "../../include/lcdb_gpu_snappy.h"

#include "lgs_launch.h"

namespace lgs {

constexpr uint32_t kChunk = 65536;   // snappy.c:28

// Records the message as the calling thread's lgs_last_error(); returns code.
int fail(int code, const char* fmt, ...);

#define LGS_HIP(call)                                                              \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(LGS_EHIP, "%s failed: %s", #call, hipGetErrorString(e_));        \
  } while (0)

#define LGS_TRY(expr)              \
  do {                             \
    int r_ = (expr);               \
    if (r_ != LGS_OK) return r_;   \
  } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

inline size_t bound_of(size_t n) { return 32 + n + n / 6; }   // snappy.c:354

// Device bytes the encoding of one 64 KiB-or-less chunk takes in a pass.
inline size_t chunk_out(uint32_t len) { return align_up(bound_of(len) + 8, 16); }

// Host staging copies (pageable caller buffers <-> the pinned arena) split
// over threads once a call moves more than 8 MB: one thread copies ~10 GB/s,
// slower than the transfers it feeds.  LGS_HOST_THREADS overrides the count
// (default: the hardware threads, at most 16).
unsigned host_threads(size_t bytes);
// f(0 .. t-1): part 0 on the caller, the others on the staging threads.
void pool_run(unsigned t, const std::function<void(unsigned)>& f);

// f(i0, i1) over [0, n) in contiguous ranges, on host_threads(bytes) threads.
template <class F>
void par_for(uint32_t n, size_t bytes, const F& f) {
  const unsigned t = host_threads(bytes);
  if (t <= 1 || n < 2 * t) {
    f(0u, n);
    return;
  }
  const uint32_t per = (n + t - 1) / t;
  pool_run(t, [&](unsigned k) {
    const uint32_t a = k * per, b = a + per < n ? a + per : n;
    if (a < b) f(a, b);
  });
}

struct Ctx {
  int device = -1;          // device this context's resources live on
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // the chunk pipeline's second stream (lazily)
  hipEvent_t done[2] = {nullptr, nullptr};
  uint8_t* d_buf = nullptr;
  size_t d_cap = 0;
  uint8_t* h_buf = nullptr; // pinned
  size_t h_cap = 0;
  uint8_t* h_dev = nullptr; // a drop-in slot's pinned arena as the device sees it
  bool fixed = false;       // a drop-in slot: arenas never grow
  uint32_t svc_idx = ~0u;   // a drop-in slot's service mailbox (kSvcMaxSlots: none)
  uint32_t svc_seq[2] = {0, 0};   // its last request per kind (encode, decode)
  bool retired = false;     // a service request timed out: never leased again
};

// The device a call from this thread runs on (made current for the thread).
int call_device(int* dev);

// The batched host API's contexts (lgs_api.cpp).
class CtxPool;
CtxPool& batch_pool();

// One context, leased for the length of a call.
class Lease {
 public:
  explicit Lease(CtxPool& p) : pool_(p) {}
  ~Lease();
  Lease(const Lease&) = delete;
  Lease& operator=(const Lease&) = delete;
  int acquire();
  Ctx& ctx() { return *c_; }

 private:
  CtxPool& pool_;
  Ctx* c_ = nullptr;
};

// Grows the context's arenas to at least these sizes; c.d_buf and c.h_buf may
// move, so a caller reads them again after every call.
int ctx_reserve(Ctx& c, size_t dev_bytes, size_t pin_bytes);

// Two streams and two events for the chunk pipeline below.
int ctx_pipeline(Ctx& c);

// Runs `chunks` independent pieces of a host call through two streams:
// stage(k) fills chunk k's own part of the pinned arena, launch(k, stream)
// enqueues its uploads, kernels and downloads, finish(k) copies its results
// out once they have arrived.  Staging chunk k+1 and finishing chunk k-1 on
// the host overlap chunk k's transfers and kernels, and consecutive chunks'
// transfers overlap each other's kernels.  Chunks use disjoint parts of the
// arenas; a stream's scratch is reused only after that stream's previous
// chunk has finished.
template <class Stage, class Launch, class Finish>
int pipeline(Ctx& c, uint32_t chunks, const Stage& stage, const Launch& launch,
             const Finish& finish) {
  LGS_TRY(ctx_pipeline(c));
  const hipStream_t st[2] = {c.stream, c.stream2};
  for (uint32_t k = 0; k < chunks; ++k) {
    stage(k);
    LGS_TRY(launch(k, st[k & 1]));
    LGS_HIP(hipEventRecord(c.done[k & 1], st[k & 1]));
    if (k >= 1) {
      LGS_HIP(hipEventSynchronize(c.done[(k - 1) & 1]));
      LGS_TRY(finish(k - 1));
    }
  }
  LGS_HIP(hipEventSynchronize(c.done[(chunks - 1) & 1]));
  return finish(chunks - 1);
}

// Chunk boundaries: [first[k], first[k+1]) over n items of `bytes` in total,
// about LGS_HOST_CHUNK_MB (default 64; 0: no chunking) each; one chunk for
// small calls.
std::vector<uint32_t> chunk_bounds(uint32_t n, size_t bytes, const uint32_t* len);

// Offsets into a staging area, 256-byte aligned.  The pinned arena and the
// device arena use the same layout, so an upload or a download is a single
// contiguous hipMemcpyAsync.
struct Layout {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at = align_up(at + bytes, 256);
    return o;
  }
};

// Query keys staged one behind the other at h_keys, 16 zero bytes after the
// last (the kernels' read slack), with their offsets from h_keys and their
// lengths: uploads of one _host call, the counterpart of entries_stage.
void stage_keys(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len, uint32_t nq,
                uint8_t* h_keys, uint64_t* koff, uint32_t* klen);

// Device memory for the length of a call, `what` naming its use in the error.
// Stream-ordered (Scratch, lgs_launch.h): freed with hipFreeAsync on s, never
// with hipFree, which synchronises the whole device and so would wait for
// resident service waves.
int scratch_alloc(std::unique_ptr<Scratch>* p, size_t bytes, hipStream_t s, const char* what);

// coding.h:169-204 on the host, for the size header only.  Returns the
// header's length in bytes (1-5), 0 if there is no valid header.
inline int read_varint32(uint32_t* v, const uint8_t* p, size_t n) {
  uint32_t acc = 0;
  unsigned sh = 0;
  for (size_t i = 0; sh <= 28 && i < n; sh += 7, ++i) {
    const uint32_t b = p[i];
    if ((b & 0x80u) == 0) {
      *v = acc | (b << sh);
      return (int)i + 1;
    }
    acc |= (b & 0x7fu) << sh;
  }
  *v = 0;
  return 0;
}

// The bloom filter's parameters, shared by the bloom API and the filter block.
inline uint32_t bloom_k(int bpk) {                        // bloom.c:35-45
  size_t k = (size_t)(bpk * 0.69);
  if (k < 1) k = 1;
  if (k > 30) k = 30;
  return (uint32_t)k;
}

inline size_t bloom_bytes(uint64_t n, int bpk) {          // bloom.c:69-80
  uint64_t bits = n * (uint64_t)bpk;
  if (bits < 64) bits = 64;
  return (size_t)((bits + 7) / 8);
}

constexpr int kMaxBitsPerKey = 1 << 16;

}  // namespace lgs
