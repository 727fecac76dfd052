// lgs_api.cpp -- host runtime and C ABI of the gfx950 Snappy codec
// (declarations, and the reference interfaces they replace:
// include/lcdb_gpu_snappy.h).
//
// HIP resources live in contexts (a non-blocking stream on one device plus a
// device arena and a pinned host arena) that are pooled per device and
// leased for the length of one call, never tied to a thread: lcdb enters the
// codec concurrently from user threads (reads) and its compaction thread
// (writes) (db_impl.c:1614-1652), and a host may create and join threads
// freely without leaking pinned memory.  Two pools:
//   * the drop-in's (ldb_snappy_*): at most LGS_DROPIN_SLOTS contexts per
//     device (default 8), each with fixed arenas of LGS_DROPIN_MB (default 4)
//     MiB that never grow -- any input size is handled in bounded passes;
//   * the batched host API's (lgs_*_host): arenas grow to the largest batch
//     a context has served, at most 16 contexts per device.
// A caller waits when its device's contexts are all leased.
//
// No compression or decompression happens on the host.  The host only moves
// bytes (pageable <-> pinned <-> device), computes the size bound
// (snappy.c:347-362) and reads the varint32 size header (snappy.c:386-399),
// and rejects on the host the streams whose header the stream's length
// cannot satisfy (an arithmetic bound, below) -- the reference rejects them
// too, so the result is the same without a device round trip.

#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/lcdb_gpu_snappy.h"

#include "lgs_block.h"
#include "lgs_launch.h"
#include "lgs_scan.h"
#include "lgs_seek.h"
#include "lgs_table_tail.h"

namespace lgs {
namespace {

constexpr uint32_t kChunk = 65536;   // snappy.c:28

thread_local char t_err[512];

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(t_err, sizeof t_err, fmt, ap);
  va_end(ap);
  return code;
}

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

size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

size_t bound_of(size_t n) { return 32 + n + n / 6; }   // snappy.c:354

// Host staging copies (pageable caller buffers <-> the pinned arena) split
// over threads once a call moves more than 8 MB: one thread copies ~10 GB/s,
// slower than the transfers it feeds.  Threads are per call (no shared pool:
// callers enter from several threads at once).  LGS_HOST_THREADS overrides
// the count (default: the hardware threads, at most 16).
unsigned host_threads(size_t bytes) {
  static const unsigned hw = [] {
    const char* e = getenv("LGS_HOST_THREADS");
    int v = e ? atoi(e) : 0;
    if (v <= 0) v = (int)std::thread::hardware_concurrency();
    if (v > 16) v = 16;
    return v > 0 ? (unsigned)v : 1u;
  }();
  return bytes < (8u << 20) ? 1u : hw;
}

// Worker threads for the staging copies: created once, never destroyed
// (like the HIP resources below), shared by every calling thread.
class Pool {
 public:
  static Pool& get() {
    static Pool* p = new Pool(host_threads(~(size_t)0));
    return *p;
  }
  // f(0 .. t-1): part 0 on the caller, the others on workers.
  void run(unsigned t, const std::function<void(unsigned)>& f) {
    std::mutex m;
    std::condition_variable cv;
    unsigned left = t - 1;
    {
      std::lock_guard<std::mutex> g(mu_);
      for (unsigned k = 1; k < t; ++k)
        q_.push_back([&, k] {
          f(k);
          std::lock_guard<std::mutex> g2(m);      // the caller's stack frame outlives this
          if (--left == 0) cv.notify_one();
        });
    }
    cv_.notify_all();
    f(0);
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return left == 0; });
  }

 private:
  explicit Pool(unsigned n) {
    for (unsigned k = 1; k < n; ++k) std::thread([this] { loop(); }).detach();
  }
  void loop() {
    for (;;) {
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !q_.empty(); });
        job = std::move(q_.front());
        q_.pop_front();
      }
      job();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
};

// f(i0, i1) over [0, n) in contiguous ranges, on host_threads(bytes) threads.
template <class F>
void par_for(uint32_t n, size_t bytes, const F& f) {
  const unsigned t = host_threads(bytes);
  if (t <= 1 || n < 2 * t) {
    f(0u, n);
    return;
  }
  const uint32_t per = (n + t - 1) / t;
  Pool::get().run(t, [&](unsigned k) {
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

// lgs_set_device() choice of the calling thread (-1: its current device).
thread_local int t_want_device = -1;

int visible_devices() {
  static const int n = [] {
    int c = 0;
    return hipGetDeviceCount(&c) == hipSuccess ? c : 0;
  }();
  return n;
}

// The device a call from this thread runs on (made current for the thread).
int call_device(int* dev) {
  const int count = visible_devices();
  if (count <= 0) return fail(LGS_ENODEV, "no HIP device visible");
  if (t_want_device < 0) {
    LGS_HIP(hipGetDevice(dev));
  } else {
    if (t_want_device >= count)
      return fail(LGS_ENODEV, "device %d not present (%d visible)", t_want_device, count);
    *dev = t_want_device;
    LGS_HIP(hipSetDevice(*dev));
  }
  if (*dev < 0 || *dev >= 64) return fail(LGS_ENODEV, "device %d out of range", *dev);
  return LGS_OK;
}

constexpr size_t kSlotDev = 64 << 10;   // a drop-in slot's device arena

size_t env_size(const char* name, size_t dflt, size_t lo, size_t hi) {
  const char* e = getenv(name);
  long v = e ? atol(e) : 0;
  size_t r = v > 0 ? (size_t)v : dflt;
  return r < lo ? lo : (r > hi ? hi : r);
}

// Drop-in slot arenas (pinned and device, each): LGS_DROPIN_MB MiB, at least
// 1 (one 64 KiB chunk's input and bound-sized output fit with room to spare).
size_t dropin_cap() {
  static const size_t v = env_size("LGS_DROPIN_MB", 4, 1, 1024) << 20;
  return v;
}
unsigned dropin_max_slots() {
  static const unsigned v = (unsigned)env_size("LGS_DROPIN_SLOTS", 8, 1, 256);
  return v;
}

// Contexts of one kind, per device.  Created on demand up to `max` per
// device; HIP resources are never freed (freeing from static destructors can
// run after the runtime is torn down at process exit).
class CtxPool {
 public:
  CtxPool(unsigned max, size_t fixed_cap) : max_(max), fixed_cap_(fixed_cap) {}

  // Lease a context on the calling thread's device; waits while all of that
  // device's contexts are leased.
  int acquire(Ctx** out) {
    int dev = -1;
    LGS_TRY(call_device(&dev));
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      std::vector<Ctx*>& fl = free_[dev];
      if (!fl.empty()) {
        *out = fl.back();
        fl.pop_back();
        return LGS_OK;
      }
      if (live_[dev] < max_) break;
      cv_.wait(lk);
    }
    ++live_[dev];
    lk.unlock();
    Ctx* c = new Ctx;
    c->device = dev;
    const int rc = create(c);
    if (rc != LGS_OK) {
      destroy_partial(c);
      lk.lock();
      --live_[dev];
      const bool others = live_[dev] > 0;
      lk.unlock();
      cv_.notify_all();
      // Out of pinned or device memory while other contexts exist: wait for
      // one of them instead of failing the call.
      if (rc == LGS_ENOMEM && others) return acquire_existing(dev, out);
      return rc;
    }
    *out = c;
    return LGS_OK;
  }

  void release(Ctx* c) {
    {
      std::lock_guard<std::mutex> g(mu_);
      if (c->retired)
        --live_[c->device];               // leaked on purpose; a new one may be made
      else
        free_[c->device].push_back(c);
    }
    cv_.notify_one();
  }

  // Bytes of pinned / device memory held by this pool's contexts.
  void footprint(size_t* pinned, size_t* device, unsigned* count) {
    std::lock_guard<std::mutex> g(mu_);
    size_t p = 0, d = 0;
    unsigned n = 0;
    for (const Ctx* c : all_) {
      p += c->h_cap;
      d += c->d_cap;
      ++n;
    }
    *pinned = p;
    *device = d;
    *count = n;
  }

  size_t fixed_cap() const { return fixed_cap_; }

 private:
  int create(Ctx* c) {
    LGS_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (fixed_cap_) {
      c->fixed = true;
      // Device memory only for the per-item arrays of an over-slot decode
      // (in-slot calls work in the mapped pinned arena).
      if (hipMalloc(&c->d_buf, kSlotDev) != hipSuccess)
        return fail(LGS_ENOMEM, "hipMalloc(%zu) failed", kSlotDev);
      c->d_cap = kSlotDev;
      // Mapped and coherent: the kernels of an in-slot call read their input
      // from it and write their output to it directly (no copies).
      if (hipHostMalloc(&c->h_buf, fixed_cap_, hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess)
        return fail(LGS_ENOMEM, "hipHostMalloc(%zu) failed", fixed_cap_);
      c->h_cap = fixed_cap_;
      void* dp = nullptr;
      LGS_HIP(hipHostGetDevicePointer(&dp, c->h_buf, 0));
      c->h_dev = (uint8_t*)dp;
    }
    std::lock_guard<std::mutex> g(mu_);
    all_.push_back(c);
    if (fixed_cap_) c->svc_idx = next_idx_[c->device]++;
    return LGS_OK;
  }
  static void destroy_partial(Ctx* c) {
    if (c->h_buf) (void)hipHostFree(c->h_buf);
    if (c->d_buf) (void)hipFree(c->d_buf);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
  }
  int acquire_existing(int dev, Ctx** out) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !free_[dev].empty(); });
    *out = free_[dev].back();
    free_[dev].pop_back();
    return LGS_OK;
  }

  const unsigned max_;
  const size_t fixed_cap_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Ctx*> free_[64];
  unsigned live_[64] = {};
  std::vector<Ctx*> all_;
  uint32_t next_idx_[64] = {};
};

CtxPool& dropin_pool() {
  static CtxPool* p = new CtxPool(dropin_max_slots(), dropin_cap());
  return *p;
}
CtxPool& batch_pool() {
  static CtxPool* p = new CtxPool(16, 0);
  return *p;
}

// One context, leased for the length of a call.
class Lease {
 public:
  explicit Lease(CtxPool& p) : pool_(p) {}
  ~Lease() {
    if (c_) pool_.release(c_);
  }
  Lease(const Lease&) = delete;
  Lease& operator=(const Lease&) = delete;
  int acquire() { return pool_.acquire(&c_); }
  Ctx& ctx() { return *c_; }

 private:
  CtxPool& pool_;
  Ctx* c_ = nullptr;
};

int ctx_reserve(Ctx& c, size_t dev_bytes, size_t pin_bytes) {
  if (c.fixed) {
    (void)dev_bytes;                        // in-slot calls work in the pinned arena
    if (pin_bytes > c.h_cap)
      return fail(LGS_EINTERNAL, "drop-in slot of %zu bytes, %zu needed", c.h_cap, pin_bytes);
    return LGS_OK;
  }
  if (dev_bytes > c.d_cap) {
    if (c.d_buf) LGS_HIP(hipFree(c.d_buf));
    c.d_buf = nullptr;
    c.d_cap = 0;
    const size_t cap = align_up(dev_bytes + dev_bytes / 4, 1 << 20);
    if (hipMalloc(&c.d_buf, cap) != hipSuccess) return fail(LGS_ENOMEM, "hipMalloc(%zu) failed", cap);
    c.d_cap = cap;
  }
  if (pin_bytes > c.h_cap) {
    if (c.h_buf) LGS_HIP(hipHostFree(c.h_buf));
    c.h_buf = nullptr;
    c.h_cap = 0;
    const size_t cap = align_up(pin_bytes + pin_bytes / 4, 1 << 20);
    if (hipHostMalloc(&c.h_buf, cap, hipHostMallocDefault) != hipSuccess)
      return fail(LGS_ENOMEM, "hipHostMalloc(%zu) failed", cap);
    c.h_cap = cap;
  }
  return LGS_OK;
}

// Two streams and two events for the chunk pipeline below.
int ctx_pipeline(Ctx& c) {
  if (c.stream2 == nullptr) LGS_HIP(hipStreamCreateWithFlags(&c.stream2, hipStreamNonBlocking));
  for (hipEvent_t& e : c.done)
    if (e == nullptr) LGS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return LGS_OK;
}

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
size_t chunk_bytes() {
  static const size_t v = [] {
    const char* e = getenv("LGS_HOST_CHUNK_MB");
    return (size_t)(e ? atoi(e) : 64) << 20;
  }();
  return v;
}

std::vector<uint32_t> chunk_bounds(uint32_t n, size_t bytes, const uint32_t* len) {
  const size_t kChunkBytes = chunk_bytes();
  std::vector<uint32_t> first{0};
  if (kChunkBytes > 0 && bytes >= 2 * kChunkBytes) {
    size_t acc = 0;
    for (uint32_t i = 0; i < n; ++i) {
      acc += len[i];
      if (acc >= kChunkBytes && i + 1 < n) {
        first.push_back(i + 1);
        acc = 0;
      }
    }
  }
  first.push_back(n);
  return first;
}

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

// coding.h:169-204 on the host, for the size header only.  Returns the
// header's length in bytes (1-5), 0 if there is no valid header.
int read_varint32(uint32_t* v, const uint8_t* p, size_t n) {
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

// LGS_DIE_EXIT=<code>: exit with that code instead of abort() (tests drive
// the failure paths in child processes without a SIGABRT on the GPU box).
[[noreturn]] void die(const char* what) {
  fprintf(stderr, "lcdb_gpu_snappy: %s failed: %s\n", what, t_err);
  fflush(stderr);
  const char* e = getenv("LGS_DIE_EXIT");
  if (e && atoi(e) > 0) _exit(atoi(e));
  abort();
}

// ---- the drop-in (ldb_snappy_encode / ldb_snappy_decode) ----
//
// Single blocks from lcdb's table builder and block reader.  Every call
// leases a drop-in slot (fixed arenas of dropin_cap() bytes), so a call
// never allocates: an input of any size goes through the slot in passes of
// whole 64 KiB chunks, which are independent (snappy.c:370-381), and the
// chunks' encodings are concatenated on the host as they come back.  The
// slot's pinned arena is mapped into the device: a pass copies the input
// into it, launches the kernel on it (input read and output written over
// PCIe, no hipMemcpy) and synchronises once.

// ---- the drop-in service (lgs_launch.h, lgs_service.h) ----
//
// One request at a time per slot: the input goes to the slot's arena at
// kSvcIn, {sequence, length} into its mailbox with one 8-byte store, and the
// call spins on the mailbox's ack (host memory) until the resident wave has
// written the output at kSvcOut.  The service kernels start on the first
// request; a request that finds its kernel gone (idle exit) relaunches it.
// LGS_DROPIN_SERVICE=0 (or lgs_set_option("service", "0")) sends every call
// through the launch path instead; so do items over kSvcMaxItem.
std::atomic<int> g_svc_enabled{[] {
  const char* e = getenv("LGS_DROPIN_SERVICE");
  return e && !strcmp(e, "0") ? 0 : 1;
}()};
std::atomic<bool> g_svc_shutdown{false};
// lgs_service_quiesce() .. lgs_service_resume(): calls take the launch path.
std::atomic<bool> g_svc_paused{false};
// svc_call's answer for a request taken back from a stopped service: the
// caller runs it through the launch path.
constexpr int kSvcWithdrawn = 1;

// Idle exit of the resident waves (LGS_SERVICE_IDLE_US, default 2 ms): a
// device-wide synchronisation waits at most this long after the last call.
uint64_t svc_idle_us() {
  static const uint64_t v = env_size("LGS_SERVICE_IDLE_US", 2000, 50, 10000000);
  return v;
}

int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

struct Service {
  std::mutex mu;
  int state = 0;                      // 0 not set up, 1 ready, -1 unavailable
  SvcMailbox* mb = nullptr;           // host view: encode [0, S), decode [S, 2S)
  SvcMailbox* mb_dev = nullptr;
  SvcControl* ctl = nullptr;          // device, one per kind
  hipStream_t stream[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  std::atomic<bool> launched[2];
  std::atomic<int64_t> last_use[2];   // steady-clock ns of the last finished request
  uint32_t nslots = 0;

  SvcMailbox* box(int kind, uint32_t idx) { return mb + (size_t)kind * kSvcMaxSlots + idx; }

  int setup() {                       // under mu
    if (state) return state > 0 ? LGS_OK : LGS_EINTERNAL;
    state = -1;
    const size_t bytes = 2 * kSvcMaxSlots * sizeof(SvcMailbox);
    if (hipHostMalloc(&mb, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
      return fail(LGS_ENOMEM, "service mailboxes: hipHostMalloc(%zu) failed", bytes);
    memset(mb, 0, bytes);
    void* dp = nullptr;
    LGS_HIP(hipHostGetDevicePointer(&dp, mb, 0));
    mb_dev = (SvcMailbox*)dp;
    if (hipMalloc(&ctl, 2 * sizeof(SvcControl)) != hipSuccess)
      return fail(LGS_ENOMEM, "service: hipMalloc failed");
    LGS_HIP(hipMemset(ctl, 0, 2 * sizeof(SvcControl)));
    // Each kind's resident kernel on a hardware queue of its own.  Streams
    // beyond GPU_MAX_HW_QUEUES share queues, and a queue runs its packets in
    // order: a relaunched encode service queued behind a decode service that
    // sustained traffic keeps alive would never start (found by
    // test_service_busy_slot_does_not_strand_another).  A stream with a CU
    // mask gets a new queue, never one from the shared pool; the mask here
    // is every CU.
    int dev = 0;
    hipDeviceProp_t prop{};
    LGS_HIP(hipGetDevice(&dev));
    LGS_HIP(hipGetDeviceProperties(&prop, dev));
    std::vector<uint32_t> cus((size_t)(prop.multiProcessorCount + 31) / 32, ~0u);
    for (int k = 0; k < 2; ++k) {
      LGS_HIP(hipExtStreamCreateWithCUMask(&stream[k], (uint32_t)cus.size(), cus.data()));
      LGS_HIP(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
      last_use[k] = 0;
      launched[k] = false;
    }
    const unsigned s = dropin_max_slots();
    nslots = s < kSvcMaxSlots ? s : kSvcMaxSlots;
    state = 1;
    return LGS_OK;
  }

  // Has the kernel of `kind` finished (or never run)?  Under mu.
  int finished(int kind, bool* gone) {
    *gone = true;
    if (!launched[kind]) return LGS_OK;
    const hipError_t q = hipEventQuery(done[kind]);
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();
      *gone = false;
      return LGS_OK;
    }
    if (q != hipSuccess) LGS_HIP(q);
    return LGS_OK;
  }

  // The kernel of `kind` running, or (re)launched -- unless the service is
  // paused (quiesce), when *gone reports whether it has finished.
  int ensure(int kind, bool* gone) {
    std::lock_guard<std::mutex> g(mu);
    *gone = false;
    if (g_svc_paused.load()) return finished(kind, gone);
    if (launched[kind]) {
      const hipError_t q = hipEventQuery(done[kind]);
      // (A pending query's hipErrorNotReady must not linger as this thread's
      // last error: the launchers return hipGetLastError().)
      if (q == hipErrorNotReady) {
        (void)hipGetLastError();
        return LGS_OK;
      }
      if (q != hipSuccess) LGS_HIP(q);
    }
    const uint64_t idle = svc_idle_us() * 100;          // 100 MHz ticks
    // The previous kernel of this kind has finished (stream order): clear its
    // closing mark for the new waves.
    LGS_HIP(hipMemsetAsync(&ctl[kind].closing, 0, sizeof(uint64_t), stream[kind]));
    LGS_HIP(kind == 0 ? launch_encode_service(mb_dev, nslots, idle, ctl, stream[0])
                      : launch_decode_service(mb_dev + kSvcMaxSlots, nslots, idle, ctl + 1,
                                              stream[1]));
    LGS_HIP(hipEventRecord(done[kind], stream[kind]));
    launched[kind] = true;
    return LGS_OK;
  }
};

Service* g_services[64] = {};
std::mutex g_services_mu;

void svc_stop_all() {
  g_svc_shutdown = true;
  for (Service* sv : g_services)
    if (sv && sv->state > 0)
      for (uint32_t i = 0; i < 2 * kSvcMaxSlots; ++i)
        __atomic_store_n(&sv->mb[i].stop, 1u, __ATOMIC_RELEASE);
}

// lgs_service_quiesce(): every service kernel stopped and finished, and
// drop-in calls sent through the launch path until lgs_service_resume(), so
// an embedding application's device-wide synchronisation (hipFree,
// hipDeviceSynchronize) does not wait for resident waves under sustained
// traffic.  A call whose request the stopped waves left unanswered takes it
// back (svc_call) and runs it through the launch path.
int svc_quiesce() {
  g_svc_paused = true;
  for (Service* sv : g_services) {
    if (!sv) continue;
    std::lock_guard<std::mutex> g(sv->mu);
    if (sv->state <= 0) continue;
    for (uint32_t i = 0; i < 2 * kSvcMaxSlots; ++i)
      __atomic_store_n(&sv->mb[i].stop, 1u, __ATOMIC_RELEASE);
    int rc = LGS_OK;
    for (int k = 0; k < 2; ++k)
      if (sv->launched[k] && hipEventSynchronize(sv->done[k]) != hipSuccess)
        rc = fail(LGS_EINTERNAL, "service quiesce: %s", hipGetErrorString(hipGetLastError()));
    for (uint32_t i = 0; i < 2 * kSvcMaxSlots; ++i)
      __atomic_store_n(&sv->mb[i].stop, 0u, __ATOMIC_RELEASE);
    for (int k = 0; k < 2; ++k) sv->launched[k] = false;
    if (rc != LGS_OK) return rc;
  }
  return LGS_OK;
}

// The calling slot's service, ready, with its arena registered; nullptr
// when the call should take the launch path.
Service* svc_for(Ctx& c) {
  if (!g_svc_enabled.load(std::memory_order_relaxed) || g_svc_shutdown.load() ||
      g_svc_paused.load() || c.svc_idx >= kSvcMaxSlots || c.device < 0 || c.device >= 64)
    return nullptr;
  Service* sv;
  {
    std::lock_guard<std::mutex> g(g_services_mu);
    sv = g_services[c.device];
    if (!sv) {
      sv = g_services[c.device] = new Service;
      static std::once_flag once;
      std::call_once(once, [] { atexit(svc_stop_all); });
    }
  }
  std::lock_guard<std::mutex> g(sv->mu);
  if (sv->setup() != LGS_OK) return nullptr;
  if (c.svc_idx >= sv->nslots) return nullptr;
  for (int k = 0; k < 2; ++k) {
    SvcMailbox* m = sv->box(k, c.svc_idx);
    if (__atomic_load_n(&m->arena, __ATOMIC_RELAXED) == 0)
      __atomic_store_n(&m->arena, (uint64_t)(uintptr_t)c.h_dev, __ATOMIC_RELEASE);
  }
  return sv;
}

// A request's input goes to the arena at kSvcIn, 16 zero bytes after it
// (the decoder's read slack).  (Round 5 staged it in host-written
// fine-grained device memory for -0.8 us, and a wave read it torn with the
// previous request's bytes: lgs_service.h.)
void svc_stage(Ctx& c, const uint8_t* xp, uint32_t n) {
  uint8_t* in = c.h_buf + kSvcIn;
  memcpy(in, xp, n);
  memset(in + n, 0, 16);
}

// Post the request staged by svc_stage and wait for it: *status and
// *out_len as the wave reported them.  kSvcWithdrawn: the service was
// stopped (quiesce) before it answered; the request is withdrawn (its ack
// written by the host, so no later wave serves it) and the caller takes the
// launch path.
int svc_call(Service& sv, Ctx& c, int kind, uint32_t len, uint32_t* status, uint32_t* out_len) {
  SvcMailbox* m = sv.box(kind, c.svc_idx);
  uint32_t seq = c.svc_seq[kind] + 1;
  if (seq == 0) seq = 1;
  c.svc_seq[kind] = seq;
  __atomic_store_n(reinterpret_cast<uint64_t*>(m), (uint64_t)seq | ((uint64_t)len << 32),
                   __ATOMIC_RELEASE);
  const int64_t t_post = now_ns();
  // Not used for over half the idle time: its kernel has likely exited.
  bool gone = false;
  if (!sv.launched[kind] ||
      t_post - sv.last_use[kind].load(std::memory_order_relaxed) > (int64_t)svc_idle_us() * 500)
    LGS_TRY(sv.ensure(kind, &gone));
  int64_t t_check = t_post;
  for (uint32_t spin = 0; __atomic_load_n(&m->ack, __ATOMIC_ACQUIRE) != seq; ++spin) {
    __builtin_ia32_pause();
    if (gone || (spin & 255) == 255) {
      const int64_t t = now_ns();
      if (gone || t - t_check > 50000) {             // 50 us: is the kernel still there?
        if (!gone) LGS_TRY(sv.ensure(kind, &gone));
        if (gone) {
          // Paused and its kernel finished: answered before it left, or
          // withdrawn now (no wave is left to write the arena).
          if (__atomic_load_n(&m->ack, __ATOMIC_ACQUIRE) == seq) break;
          __atomic_store_n(&m->ack, seq, __ATOMIC_RELEASE);
          return kSvcWithdrawn;
        }
        t_check = t;
      }
      if (t - t_post > 20000000000ll) {
        // The wave may still answer later and write into the arena: stop it
        // and retire the slot, so no later lessee shares the arena with it.
        __atomic_store_n(&m->stop, 1u, __ATOMIC_RELEASE);
        c.retired = true;
        return fail(LGS_EINTERNAL, "drop-in service: no answer in 20 s");
      }
    }
  }
  *status = __atomic_load_n(&m->status, __ATOMIC_RELAXED);
  *out_len = __atomic_load_n(&m->out_len, __ATOMIC_RELAXED);
  sv.last_use[kind].store(now_ns(), std::memory_order_relaxed);
  return LGS_OK;
}

// Device bytes one 64 KiB-or-less chunk takes in a pass.
constexpr size_t kChunkIn = kChunk + 16;                         // its input
size_t chunk_out(uint32_t len) { return align_up(bound_of(len) + 8, 16); }

int encode_one(uint8_t* zp, const uint8_t* xp, size_t xn, size_t* written) {
  if (xn > 0x7fffffffu) return fail(LGS_EINVAL, "input of %zu bytes too large", xn);
  Lease lease(dropin_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  const uint32_t n = (uint32_t)xn;
  if (n <= kSvcMaxItem) {
    if (Service* sv = svc_for(c)) {                              // a resident wave
      svc_stage(c, xp, n);
      uint32_t st = 0, olen = 0;
      const int rc = svc_call(*sv, c, 0, n, &st, &olen);
      if (rc == LGS_OK) {
        if (st != 1 || olen > bound_of(n))
          return fail(LGS_EINTERNAL, "service encode: status %u, %u bytes", st, olen);
        memcpy(zp, c.h_buf + kSvcOut, olen);
        *written = olen;
        return LGS_OK;
      }
      if (rc != kSvcWithdrawn) return rc;
    }
  }
  // snappy.c:370-381: full 64 KiB chunks, then the remainder (if any);
  // a zero-length input is one empty item (just the varint header).
  const uint32_t nit = n <= kChunk ? 1u : (n + kChunk - 1) / kChunk;
  // Chunks per pass: per chunk its input, its output slot and 32 bytes of
  // per-item arrays, plus 7 x 256 of alignment slack.
  const size_t per = kChunkIn + chunk_out(kChunk) + 32 + 64;
  const uint32_t kmax = (uint32_t)((c.h_cap - 8 * 256) / per);
  if (kmax == 0) return fail(LGS_EINTERNAL, "drop-in slot of %zu bytes too small", c.h_cap);
  uint8_t* const h = c.h_buf;
  uint8_t* const hd = c.h_dev;
  size_t total = 0;
  for (uint32_t j0 = 0; j0 < nit; j0 += kmax) {
    const uint32_t k = nit - j0 < kmax ? nit - j0 : kmax;
    const size_t at = (size_t)j0 * kChunk;                      // input offset of the pass
    const size_t in_bytes = n - at < (size_t)k * kChunk ? n - at : (size_t)k * kChunk;
    Layout L;                                                    // upload | download
    const size_t o_in = L.take(in_bytes + 16);
    const size_t o_ioff = L.take(8 * (size_t)k);
    const size_t o_ilen = L.take(4 * (size_t)k);
    const size_t o_ooff = L.take(8 * (size_t)k);
    const size_t o_hdr = L.take(4 * (size_t)k);
    const size_t up_end = L.at;
    const size_t o_olen = L.take(4 * (size_t)k);
    size_t out_bytes = 0;
    for (uint32_t j = 0; j < k; ++j) {
      const size_t off = (size_t)j * kChunk;
      const uint32_t len = (uint32_t)(in_bytes - off < kChunk ? in_bytes - off : kChunk);
      out_bytes += chunk_out(len);
    }
    const size_t o_out = L.take(out_bytes);
    const size_t down_end = L.at;
    LGS_TRY(ctx_reserve(c, down_end, down_end));

    memcpy(h + o_in, xp + at, in_bytes);
    memset(h + o_in + in_bytes, 0, 16);
    uint64_t* ioff = (uint64_t*)(h + o_ioff);
    uint32_t* ilen = (uint32_t*)(h + o_ilen);
    uint64_t* ooff = (uint64_t*)(h + o_ooff);
    uint32_t* hdr = (uint32_t*)(h + o_hdr);
    size_t oa = o_out;
    for (uint32_t j = 0; j < k; ++j) {
      const size_t off = (size_t)j * kChunk;
      ilen[j] = (uint32_t)(in_bytes - off < kChunk ? in_bytes - off : kChunk);
      ioff[j] = o_in + off;
      ooff[j] = oa;
      oa += chunk_out(ilen[j]);
      hdr[j] = j0 + j == 0 ? n : 0xffffffffu;                    // snappy.c:368
    }
    (void)up_end;
    EncodeArgs a{hd, (const uint64_t*)(hd + o_ioff), (const uint32_t*)(hd + o_ilen), hd,
                 (const uint64_t*)(hd + o_ooff), (uint32_t*)(hd + o_olen),
                 (const uint32_t*)(hd + o_hdr), nullptr, k, nullptr};
    if (k == 1) a.one = Item1{ioff[0], ooff[0], ilen[0], hdr[0], 1};
    LGS_HIP(launch_encode(a, k == 1 ? ilen[0] : kChunk, c.stream));
    LGS_HIP(hipStreamSynchronize(c.stream));
    const uint32_t* olen = (const uint32_t*)(h + o_olen);
    for (uint32_t j = 0; j < k; ++j) {
      if (olen[j] > chunk_out(ilen[j]))
        return fail(LGS_EINTERNAL, "encoded chunk of %u bytes exceeds its bound", olen[j]);
      memcpy(zp + total, h + ooff[j], olen[j]);
      total += olen[j];
    }
  }
  if (total > bound_of(n)) return fail(LGS_EINTERNAL, "encoded length %zu exceeds bound", total);
  *written = total;
  return LGS_OK;
}

// The largest output an in-slot decode produces: the wave decoder's biggest
// LDS class (lgs_decode.hip kDecCap2).
constexpr uint32_t kInSlotDecodeMax = 66048;

// Host-side reference rejects, from the header and the stream length only
// (snappy.c:201-341): with m stream bytes after a header of `want`,
//   * want == 0: the reference accepts exactly when m == 0 (every tag either
//     produces >= 1 byte, failing len > zn, or is a copy failing :323);
//   * a COPY2 tag (3 bytes) yields at most 64 bytes, every other tag less
//     per byte, so 3 * want > 64 * m can never reach zn == 0 (:337);
//   * a tag consumes at most 6 bytes per byte it yields (a literal of one
//     byte with a 4-byte length: 1 + 4 + 1), so m > 6 * want must run out
//     of output first (:263, :323).
// Returns 1 (accept), 0 (reject) or -1 (the device decides).
int host_verdict(uint32_t want, size_t m) {
  if (want == 0) return m == 0 ? 1 : 0;
  if (3 * (uint64_t)want > 64 * (uint64_t)m) return 0;
  if ((uint64_t)m > 6 * (uint64_t)want) return 0;
  return -1;
}

// Device memory for an over-slot decode.  A valid stream must never come
// back as corrupt because memory is short for a moment (lcdb
// would turn that 0 into a lasting LDB_CORRUPTION background error), so a
// failed hipMalloc is tried 13 times, 12 sleeps from 0.5 ms doubling to a
// 256 ms cap between them (about 1 s in all), before the call fails -- and then ldb_snappy_decode aborts with a
// diagnostic, as on any other device failure.  Test hook:
// lgs_set_option("inject_alloc_failures", "N") makes the next N attempts
// fail as if the device were out of memory.
std::atomic<int> g_inject_alloc_failures{0};

// Stream-ordered (Scratch, lgs_launch.h): freed with hipFreeAsync on the
// slot's stream, never with hipFree, which synchronises the whole device and
// so would wait for resident service waves.
int big_alloc(std::unique_ptr<Scratch>* p, size_t bytes, uint32_t want, hipStream_t s) {
  unsigned wait_us = 500;
  for (int attempt = 0;; ++attempt) {
    int inj = g_inject_alloc_failures.load();
    bool injected = false;
    while (inj > 0 && !(injected = g_inject_alloc_failures.compare_exchange_weak(inj, inj - 1))) {
    }
    if (!injected) {
      p->reset(new Scratch(bytes, s));
      if ((*p)->status() == hipSuccess) return LGS_OK;
      p->reset();
      (void)hipGetLastError();
    }
    if (attempt == 12)
      return fail(LGS_ENOMEM, "hipMalloc(%zu) for a %u-byte block failed %d times", bytes, want,
                  attempt + 1);
    std::this_thread::sleep_for(std::chrono::microseconds(wait_us));
    wait_us = wait_us < 256000 ? 2 * wait_us : wait_us;
  }
}

// Decode one host block on the GPU.  *ok = reference decode result.
int decode_one(uint8_t* zp, const uint8_t* xp, size_t xn, int* ok) {
  *ok = 0;
  uint32_t want = 0;
  const int hl = read_varint32(&want, xp, xn);
  if (hl == 0 || want > 0x7fffffffu) return LGS_OK;            // snappy.c:405-409
  const int hv = host_verdict(want, xn - (size_t)hl);
  if (hv >= 0) {
    *ok = hv;
    return LGS_OK;
  }
  // Blocks are addressed with 32-bit lengths on the device.  A stream this
  // long passed host_verdict (want >= xn / 6 > 700 MB) and may be valid, so
  // it is not reported as corrupt: the call fails as unsupported.  (lcdb's
  // blocks are 4 KiB - a few MiB; format.c reads a block's bytes from the
  // file before decoding, so only a real multi-GiB block gets here.)
  if (xn > 0xffffffffu)
    return fail(LGS_EINVAL, "a %zu-byte stream exceeds the device decoder's 4 GiB limit", xn);
  const uint32_t n = (uint32_t)xn;
  Lease lease(dropin_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  uint8_t* const h = c.h_buf;
  if (want <= kSvcMaxItem && (size_t)n + 16 <= kSvcOut - kSvcIn) {
    if (Service* sv = svc_for(c)) {                              // a resident wave
      svc_stage(c, xp, n);
      uint32_t st = 0, olen = 0;
      const int rc = svc_call(*sv, c, 1, n, &st, &olen);
      if (rc == LGS_OK) {
        if (st == LGS_ST_OK && olen != want)
          return fail(LGS_EINTERNAL, "service decode: %u bytes for a %u-byte header", olen, want);
        if (st == LGS_ST_OK) memcpy(zp, h + kSvcOut, want);
        *ok = st == LGS_ST_OK;
        return LGS_OK;
      }
      if (rc != kSvcWithdrawn) return rc;
    }
  }

  Layout L;
  const size_t o_in = L.take((size_t)n + 16);
  const size_t o_ioff = L.take(8);
  const size_t o_ilen = L.take(4);
  const size_t o_ooff = L.take(8);
  const size_t o_ocap = L.take(4);
  const size_t up_end = L.at;
  const size_t o_st = L.take(4);
  const size_t o_olen = L.take(4);
  const size_t o_out = L.take((size_t)want + 16);
  const size_t down_end = L.at;
  if (down_end <= c.h_cap && want <= kInSlotDecodeMax) {
    // In the slot: the kernel reads the stream from the mapped pinned arena
    // and writes status, length and output there; one synchronisation.
    // (Outputs over the LDS classes decode straight against global memory,
    // one fenced round trip per copy: those take device memory below.)
    uint8_t* const hd = c.h_dev;
    (void)up_end;
    memcpy(h + o_in, xp, n);
    memset(h + o_in + n, 0, 16);
    *(uint64_t*)(h + o_ioff) = o_in;
    *(uint32_t*)(h + o_ilen) = n;
    *(uint64_t*)(h + o_ooff) = o_out;
    *(uint32_t*)(h + o_ocap) = want;
    DecodeArgs a{hd, (const uint64_t*)(hd + o_ioff), (const uint32_t*)(hd + o_ilen), hd,
                 (const uint64_t*)(hd + o_ooff), (const uint32_t*)(hd + o_ocap),
                 (uint32_t*)(hd + o_olen), hd + o_st, nullptr, 1, nullptr};
    a.one = Item1{o_in, o_out, n, want, 1};
    LGS_HIP(launch_decode(a, want, c.stream));
    LGS_HIP(hipStreamSynchronize(c.stream));
    const uint8_t st = h[o_st];
    if (st == LGS_ST_OK) memcpy(zp, h + o_out, want);
    *ok = st == LGS_ST_OK;
    return LGS_OK;
  }
  // Larger than the slot or than the LDS classes (multi-MiB index blocks):
  // device memory for this call only, the stream uploaded straight from the
  // caller's (pageable) buffer, and the output downloaded into zp only once
  // the status says ok.
  std::unique_ptr<Scratch> guard;
  const size_t big_bytes = align_up((size_t)n + 16, 256) + align_up((size_t)want + 16, 256);
  LGS_TRY(big_alloc(&guard, big_bytes, want, c.stream));
  uint8_t* const big = (uint8_t*)guard->get();
  uint8_t* const d_in = big;
  uint8_t* const d_out = big + align_up((size_t)n + 16, 256);
  Layout M;                                                      // per-item arrays, in the slot
  const size_t m_ioff = M.take(8), m_ilen = M.take(4), m_ooff = M.take(8), m_ocap = M.take(4);
  const size_t m_up = M.at;
  const size_t m_st = M.take(4), m_olen = M.take(4);
  const size_t m_down = M.at;
  uint8_t* const d = c.d_buf;
  *(uint64_t*)(h + m_ioff) = 0;
  *(uint32_t*)(h + m_ilen) = n;
  *(uint64_t*)(h + m_ooff) = 0;
  *(uint32_t*)(h + m_ocap) = want;
  LGS_HIP(hipMemcpyAsync(d_in, xp, n, hipMemcpyHostToDevice, c.stream));
  LGS_HIP(hipMemsetAsync(d_in + n, 0, 16, c.stream));
  LGS_HIP(hipMemcpyAsync(d, h, m_up, hipMemcpyHostToDevice, c.stream));
  DecodeArgs a{d_in, (const uint64_t*)(d + m_ioff), (const uint32_t*)(d + m_ilen), d_out,
               (const uint64_t*)(d + m_ooff), (const uint32_t*)(d + m_ocap),
               (uint32_t*)(d + m_olen), d + m_st, nullptr, 1, nullptr};
  LGS_HIP(launch_decode(a, want, c.stream));
  LGS_HIP(hipMemcpyAsync(h + m_st, d + m_st, m_down - m_st, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  if (h[m_st] == LGS_ST_OK) {
    LGS_HIP(hipMemcpyAsync(zp, d_out, want, hipMemcpyDeviceToHost, c.stream));
    LGS_HIP(hipStreamSynchronize(c.stream));
    *ok = 1;
  }
  return LGS_OK;
}

// Kernel options: lgs_set_option(), initial values from the environment.
Options& options_init() {
  static Options* o = [] {
    Options* v = new Options;
    const char* dk = getenv("LGS_DECODE_KERNEL");
    if (dk && !strcmp(dk, "ring")) v->decoder = kDecRing;
    if (dk && !strcmp(dk, "ring32")) v->decoder = kDecRing32;
    if (dk && !strcmp(dk, "wave")) v->decoder = kDecWave;
#ifdef LGS_PROBE_DECODERS
    if (dk && !strcmp(dk, "chain")) v->decoder = kDecChain;
    if (dk && !strcmp(dk, "group")) v->decoder = kDecGroup;
    const char* wg = getenv("LGS_WIDE_DECODER");
    if (wg && !strcmp(wg, "group")) v->wide = kWideGroup;
    if (dk && !strcmp(dk, "quad")) v->decoder = kDecQuad;
    if (dk && !strcmp(dk, "ops")) v->decoder = kDecOps;
    const char* wd = getenv("LGS_WIDE_DECODER");
    if (wd && !strcmp(wd, "trips")) v->wide = kWideTrips;
#endif
#ifndef LGS_PROBE_DECODERS
    // The decoders that lost their A/B exist in the probe library only: say
    // so rather than silently measuring the default.
    const char* wd0 = getenv("LGS_WIDE_DECODER");
    if ((dk && (!strcmp(dk, "quad") || !strcmp(dk, "ops") || !strcmp(dk, "group") ||
                !strcmp(dk, "chain"))) ||
        (wd0 && (!strcmp(wd0, "trips") || !strcmp(wd0, "group"))))
      fprintf(stderr,
              "lcdb_gpu_snappy: LGS_DECODE_KERNEL=%s LGS_WIDE_DECODER=%s names a probe-library "
              "decoder; this library uses its default decoders\n",
              dk ? dk : "", wd0 ? wd0 : "");
#endif
    const char* vo = getenv("LGS_VERIFY_OVERLAP");
    if (vo && !strcmp(vo, "0")) v->verify_overlap = 0;
    const char* ns = getenv("LGS_NO_SPLIT");
    if (ns && *ns && strcmp(ns, "0")) v->split = 0;
    return v;
  }();
  return *o;
}

}  // namespace

int set_error(int code, const char* msg) { return fail(code, "%s", msg); }

Options& options() { return options_init(); }

// off[i] = i * stride (lgs_table.hip; declared here, not in lgs_launch.h,
// whose text keys the codec kernels' traffic figures).
hipError_t launch_fill_stride(uint64_t* off, uint64_t stride, uint32_t n, hipStream_t s);
// check_kernel's checks with one lane per handle, no CRC (lgs_table.hip;
// declared here for the same reason).
hipError_t launch_check_lane(const CheckArgs& a, hipStream_t s);

}  // namespace lgs

using namespace lgs;

extern "C" {

// ---- drop-in (src/util/snappy.h:28-38) ----

int ldb_snappy_encode_size(size_t* zn, size_t xn) {   // snappy.c:347-362
  if (xn > 0x7fffffff) return 0;
  const size_t n = bound_of(xn);
  if (n > 0x7fffffff) return 0;
  *zn = n;
  return 1;
}

size_t ldb_snappy_encode(uint8_t* zp, const uint8_t* xp, size_t xn) {
  // lcdb's encode path has no error return (table_builder.c:182-188): a
  // failure here is a lost device or a broken runtime, so abort loudly.
  size_t written = 0;
  if (encode_one(zp, xp, xn, &written) != LGS_OK) die("ldb_snappy_encode");
  return written;
}

int ldb_snappy_decode_size(size_t* zn, const uint8_t* xp, size_t xn) {   // snappy.c:386-399
  uint32_t v;
  if (!read_varint32(&v, xp, xn)) return 0;
  if (v > 0x7fffffffu) return 0;
  *zn = v;
  return 1;
}

int ldb_snappy_decode(uint8_t* zp, const uint8_t* xp, size_t xn) {
  // format.c:237-251 turns 0 into LDB_CORRUPTION, so 0 means exactly the
  // reference's 0.  A call that cannot run (device memory still short after
  // big_alloc's retries, a lost device, a stream beyond the device's 4 GiB
  // addressing) is not a corrupt block: it aborts with a diagnostic.
  int ok = 0;
  if (decode_one(zp, xp, xn, &ok) != LGS_OK) die("ldb_snappy_decode");
  return ok;
}

// ---- drop-in footprint and kernel options ----

int lgs_dropin_footprint(size_t* pinned, size_t* device, uint32_t* slots, size_t* slot_bytes) {
  if (!pinned || !device || !slots || !slot_bytes) return fail(LGS_EINVAL, "NULL argument");
  unsigned n = 0;
  dropin_pool().footprint(pinned, device, &n);
  *slots = n;
  *slot_bytes = dropin_pool().fixed_cap();
  return LGS_OK;
}

int lgs_service_quiesce(void) { return lgs::svc_quiesce(); }

int lgs_service_resume(void) {
  lgs::g_svc_paused = false;
  return LGS_OK;
}

int lgs_set_option(const char* name, const char* value) {
  if (!name || !value) return fail(LGS_EINVAL, "NULL argument");
  Options& o = options();
  if (!strcmp(name, "decoder")) {
    if (!strcmp(value, "auto") || !*value) o.decoder = kDecAuto;
    else if (!strcmp(value, "ring")) o.decoder = kDecRing;
    else if (!strcmp(value, "ring32")) o.decoder = kDecRing32;
    else if (!strcmp(value, "wave")) o.decoder = kDecWave;
#ifdef LGS_PROBE_DECODERS
    else if (!strcmp(value, "chain")) o.decoder = kDecChain;
    else if (!strcmp(value, "group")) o.decoder = kDecGroup;
    // The decoders that lost their A/B exist in the probe library only
    // (lgs_decode_probe.hip); the product rejects them.
    else if (!strcmp(value, "quad")) o.decoder = kDecQuad;
    else if (!strcmp(value, "ops")) o.decoder = kDecOps;
#endif
    else return fail(LGS_EINVAL, "decoder '%s' (auto, ring or wave)", value);
    return LGS_OK;
  }
  if (!strcmp(name, "inject_alloc_failures")) {   // test hook (big_alloc)
    char* end = nullptr;
    const long v = strtol(value, &end, 10);
    if (!*value || *end || v < 0 || v > 1000000)
      return fail(LGS_EINVAL, "inject_alloc_failures '%s' (0..1000000)", value);
    g_inject_alloc_failures = (int)v;
    return LGS_OK;
  }
  if (!strcmp(name, "wide")) {
    if (!strcmp(value, "walk") || !*value) o.wide = kWideWalk;
#ifdef LGS_PROBE_DECODERS
    else if (!strcmp(value, "group")) o.wide = kWideGroup;
    else if (!strcmp(value, "trips")) o.wide = kWideTrips;
#endif
    else return fail(LGS_EINVAL, "wide '%s' (walk)", value);
    return LGS_OK;
  }
  if (!strcmp(name, "service")) {   // the drop-in's resident waves (LGS_DROPIN_SERVICE)
    if (!strcmp(value, "1")) g_svc_enabled = 1;
    else if (!strcmp(value, "0")) g_svc_enabled = 0;
    else return fail(LGS_EINVAL, "service '%s' (0 or 1)", value);
    return LGS_OK;
  }
  if (!strcmp(name, "verify_overlap")) {   // table reads: CRC pass beside the decoder
    if (!strcmp(value, "1")) o.verify_overlap = 1;
    else if (!strcmp(value, "0")) o.verify_overlap = 0;
    else return fail(LGS_EINVAL, "verify_overlap '%s' (0 or 1)", value);
    return LGS_OK;
  }
  if (!strcmp(name, "split")) {
    if (!strcmp(value, "1")) o.split = 1;
    else if (!strcmp(value, "0")) o.split = 0;
    else return fail(LGS_EINVAL, "split '%s' (0 or 1)", value);
    return LGS_OK;
  }
  return fail(LGS_EINVAL, "unknown option '%s'", name);
}

// ---- batched API ----

size_t lgs_encode_bound(size_t n) { return bound_of(n); }

int lgs_encode_batch_dev(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                         uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len,
                         uint32_t n, uint32_t max_in_len, void* stream) {
  if (n == 0) return LGS_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len)
    return fail(LGS_EINVAL, "NULL argument");
  if (max_in_len > 0x7fffffffu) return fail(LGS_EINVAL, "max_in_len %u too large", max_in_len);
  EncodeArgs a{d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_len, nullptr, nullptr, n, nullptr};
  LGS_HIP(launch_encode(a, max_in_len, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_decode_batch_dev(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                         uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                         uint32_t* d_out_len, uint8_t* d_status, uint32_t n,
                         uint32_t max_out_cap, void* stream) {
  if (n == 0) return LGS_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len ||
      !d_status)
    return fail(LGS_EINVAL, "NULL argument");
  DecodeArgs a{d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status,
               nullptr, n, nullptr};
  LGS_HIP(launch_decode(a, max_out_cap, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_encode_batch_host(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                          uint8_t* out, const uint64_t* out_off, uint32_t* out_len, uint32_t n) {
  if (n == 0) return LGS_OK;
  if (!in || !in_off || !in_len || !out || !out_off || !out_len)
    return fail(LGS_EINVAL, "NULL argument");
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  size_t in_total = 0, out_total = 0;
  uint32_t max_in = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (in_len[i] > 0x7fffffffu) return fail(LGS_EINVAL, "block %u too large", i);
    in_total += align_up(in_len[i], 16);
    out_total += align_up(bound_of(in_len[i]), 16);
    if (in_len[i] > max_in) max_in = in_len[i];
  }
  // The encodings land in bound-spaced device slots; a scan of their lengths
  // and a pack kernel then put them end to end, so only the compressed bytes
  // cross PCIe (C2: 153 MB instead of 316 MB of slots).  The packed region
  // comes back into the pinned slot region, which it never exceeds.
  Layout L;
  const size_t o_in = L.take(in_total + 16);
  const size_t o_ioff = L.take(8 * (size_t)n);
  const size_t o_ilen = L.take(4 * (size_t)n);
  const size_t o_ooff = L.take(8 * (size_t)n);
  const size_t up_end = L.at;
  const size_t o_olen = L.take(4 * (size_t)n);
  const size_t o_poff = L.take(8 * (size_t)n);
  const size_t o_pend = L.take(8);
  const size_t meta_end = L.at;
  const size_t o_out = L.take(out_total + 16);
  const size_t down_end = L.at;
  const size_t o_part = L.take(8 * scan_parts(n) + 8);          // device only
  const size_t o_pack = L.take(out_total + 16);                 // device only
  LGS_TRY(ctx_reserve(c, L.at, down_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  uint64_t* ioff = (uint64_t*)(h + o_ioff);
  uint32_t* ilen = (uint32_t*)(h + o_ilen);
  uint64_t* ooff = (uint64_t*)(h + o_ooff);
  size_t ia = o_in, oa = o_out;
  for (uint32_t i = 0; i < n; ++i) {
    ioff[i] = ia;
    ilen[i] = in_len[i];
    ooff[i] = oa;
    ia += align_up(in_len[i], 16);
    oa += align_up(bound_of(in_len[i]), 16);
  }
  par_for(n, in_total, [&](uint32_t i0, uint32_t i1) {
    for (uint32_t i = i0; i < i1; ++i) memcpy(h + ioff[i], in + in_off[i], in_len[i]);
  });
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, c.stream));
  EncodeArgs a{d, (const uint64_t*)(d + o_ioff), (const uint32_t*)(d + o_ilen), d,
               (const uint64_t*)(d + o_ooff), (uint32_t*)(d + o_olen), nullptr, nullptr, n, nullptr};
  LGS_HIP(launch_encode(a, max_in, c.stream));
  LGS_HIP(launch_scan(2, nullptr, (const uint32_t*)(d + o_olen), (uint64_t*)(d + o_part), 0,
                      (uint64_t*)(d + o_poff), (uint64_t*)(d + o_pend), n, c.stream));
  LGS_HIP(launch_pack(d, (const uint64_t*)(d + o_ooff), (const uint32_t*)(d + o_olen),
                      d + o_pack, (const uint64_t*)(d + o_poff), n, c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_olen, d + o_olen, meta_end - o_olen, hipMemcpyDeviceToHost,
                         c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  const uint64_t packed = *(const uint64_t*)(h + o_pend);
  if (packed > out_total) return fail(LGS_EINTERNAL, "packed encodings exceed their slots");
  LGS_HIP(hipMemcpyAsync(h + o_out, d + o_pack, packed, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  const uint32_t* olen = (const uint32_t*)(h + o_olen);
  const uint64_t* poff = (const uint64_t*)(h + o_poff);
  par_for(n, packed, [&](uint32_t i0, uint32_t i1) {
    for (uint32_t i = i0; i < i1; ++i) {
      memcpy(out + out_off[i], h + o_out + poff[i], olen[i]);
      out_len[i] = olen[i];
    }
  });
  return LGS_OK;
}

int lgs_decode_batch_host(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                          uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                          uint32_t* out_len, uint8_t* status, uint32_t n) {
  if (n == 0) return LGS_OK;
  if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status)
    return fail(LGS_EINVAL, "NULL argument");
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  size_t in_total = 0, out_total = 0;
  uint32_t max_cap = 0;
  for (uint32_t i = 0; i < n; ++i) {
    in_total += align_up(in_len[i], 16);
    out_total += align_up(out_cap[i], 16);
    if (out_cap[i] > max_cap) max_cap = out_cap[i];
  }
  Layout L;
  const size_t o_in = L.take(in_total + 16);
  const size_t o_ioff = L.take(8 * (size_t)n);
  const size_t o_ilen = L.take(4 * (size_t)n);
  const size_t o_ooff = L.take(8 * (size_t)n);
  const size_t o_ocap = L.take(4 * (size_t)n);
  const size_t up_end = L.at;
  const size_t o_st = L.take((size_t)n);
  const size_t o_olen = L.take(4 * (size_t)n);
  const size_t o_out = L.take(out_total + 16);
  const size_t down_end = L.at;
  LGS_TRY(ctx_reserve(c, down_end, down_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  uint64_t* ioff = (uint64_t*)(h + o_ioff);
  uint32_t* ilen = (uint32_t*)(h + o_ilen);
  uint64_t* ooff = (uint64_t*)(h + o_ooff);
  uint32_t* ocap = (uint32_t*)(h + o_ocap);
  size_t ia = o_in, oa = o_out;
  for (uint32_t i = 0; i < n; ++i) {
    ioff[i] = ia;
    ilen[i] = in_len[i];
    ooff[i] = oa;
    ocap[i] = out_cap[i];
    ia += align_up(in_len[i], 16);
    oa += align_up(out_cap[i], 16);
  }
  par_for(n, in_total, [&](uint32_t i0, uint32_t i1) {
    for (uint32_t i = i0; i < i1; ++i) memcpy(h + ioff[i], in + in_off[i], in_len[i]);
  });
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, c.stream));
  DecodeArgs a{d, (const uint64_t*)(d + o_ioff), (const uint32_t*)(d + o_ilen), d,
               (const uint64_t*)(d + o_ooff), (const uint32_t*)(d + o_ocap),
               (uint32_t*)(d + o_olen), d + o_st, nullptr, n, nullptr};
  LGS_HIP(launch_decode(a, max_cap, c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_st, d + o_st, down_end - o_st, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  const uint32_t* olen = (const uint32_t*)(h + o_olen);
  par_for(n, out_total, [&](uint32_t i0, uint32_t i1) {
    for (uint32_t i = i0; i < i1; ++i) {
      status[i] = h[o_st + i];
      out_len[i] = olen[i];
      if (status[i] == LGS_ST_OK) memcpy(out + out_off[i], h + ooff[i], olen[i]);
    }
  });
  return LGS_OK;
}

// ---- SSTable block framing (kernels: lgs_table.hip) ----

int lgs_crc32c_batch_dev(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                         const uint8_t* d_type, int masked, uint32_t* d_crc, uint32_t n,
                         void* stream) {
  if (n == 0) return LGS_OK;
  if (!d_in || !d_in_off || !d_in_len || !d_crc) return fail(LGS_EINVAL, "NULL argument");
  LGS_HIP(launch_crc(d_in, d_in_off, d_in_len, d_type, masked, d_crc, n, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_hbm_copy_dev(void* d_dst, const void* d_src, size_t bytes, void* stream) {
  if (bytes == 0) return LGS_OK;
  if (!d_dst || !d_src) return fail(LGS_EINVAL, "NULL argument");
  if (((uintptr_t)d_dst | (uintptr_t)d_src | bytes) & 15)
    return fail(LGS_EINVAL, "hbm copy needs 16-byte aligned pointers and length");
  LGS_HIP(launch_hbm_copy(d_dst, d_src, bytes, (hipStream_t)stream));
  return LGS_OK;
}

namespace {

// Device scratch of the write path (offsets from the scratch base).
struct WriteScratch {
  size_t enc_off, enc_len, part, foff, enc, enc_cap, total;
  WriteScratch(uint32_t n, uint64_t raw_total) {
    Layout L;
    enc_off = L.take(8 * (size_t)n);
    enc_len = L.take(4 * (size_t)n);
    part = L.take(8 * scan_parts(n) + 8);
    foff = L.take(8 * (size_t)n);
    // >= the sum of 16-aligned bounds, with 1/8 more so that near-uniform
    // blocks (lcdb's: every one within 1/8 of the mean) take one stride
    // (table_write: one fill kernel instead of a three-kernel scan).
    const uint64_t bounds = raw_total + raw_total / 6;
    enc_cap = 48 * (size_t)n + bounds + bounds / 8 + 64;
    enc = L.take(enc_cap);
    total = L.at;
  }
};

struct ReadScratch {
  size_t in_off, len, off, cap, olen, st, bad, dummy, total;
  explicit ReadScratch(uint32_t n) {
    Layout L;
    bad = L.take((size_t)n);
    in_off = L.take(8 * (size_t)n);
    len = L.take(4 * (size_t)n);
    off = L.take(8 * (size_t)n);
    cap = L.take(4 * (size_t)n);
    olen = L.take(4 * (size_t)n);
    st = L.take((size_t)n);
    dummy = L.take(64);
    total = L.at;
  }
};

static int table_write(const uint8_t* d_raw, const uint64_t* d_raw_off, const uint32_t* d_raw_len,
                uint32_t n, uint32_t max_raw_len, int compression, uint64_t base, uint8_t* d_file,
                uint64_t* d_handle_off, uint64_t* d_handle_size, uint64_t* d_end, uint8_t* scratch,
                const WriteScratch& W, hipStream_t s) {
  uint64_t* enc_off = (uint64_t*)(scratch + W.enc_off);
  uint32_t* enc_len = (uint32_t*)(scratch + W.enc_len);
  uint64_t* part = (uint64_t*)(scratch + W.part);
  uint64_t* foff = (uint64_t*)(scratch + W.foff);
  uint8_t* enc = scratch + W.enc;
  const bool snappy = compression == LGS_SNAPPY_COMPRESSION;
  if (snappy) {                       // table_builder.c:176-188, every block at once
    // Encode slots: one stride for all when n of the largest block's bound
    // fit (lcdb's near-uniform blocks: one fill instead of a three-kernel
    // scan), else the scan of every block's own bound.
    const uint64_t stride = (32 + (uint64_t)max_raw_len + max_raw_len / 6 + 15) & ~15ull;
    if (stride * n <= W.enc_cap)
      LGS_HIP(launch_fill_stride(enc_off, stride, n, s));
    else
      LGS_HIP(launch_scan(0, d_raw_len, nullptr, part, 0, enc_off, nullptr, n, s));
    EncodeArgs a{d_raw, d_raw_off, d_raw_len, enc, enc_off, enc_len, nullptr, nullptr, n, nullptr};
    LGS_HIP(launch_encode(a, max_raw_len, s));
  }
  // File offsets of the framed blocks (table_builder.c:150), then the blocks.
  LGS_HIP(launch_scan(1, d_raw_len, snappy ? enc_len : nullptr, part, base, foff, d_end, n, s));
  FrameArgs f{d_raw, d_raw_off, d_raw_len, enc, enc_off, snappy ? enc_len : nullptr,
              d_file, base, foff, d_handle_off, d_handle_size, n};
  LGS_HIP(launch_frame(f, s));
  return LGS_OK;
}

// A second stream per device and calling thread for the table reader's
// checksum pass (one per device for the whole process would serialise
// independent callers' passes on it).
static hipStream_t aux_stream() {
  thread_local hipStream_t s[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!s[dev] && hipStreamCreateWithFlags(&s[dev], hipStreamNonBlocking) != hipSuccess)
    s[dev] = nullptr;
  return s[dev];
}

struct EventPair {
  hipEvent_t e[2] = {nullptr, nullptr};
  ~EventPair() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);   // released once the work it marks completes
  }
};

static int table_read(const uint8_t* d_file, uint64_t file_len, const uint64_t* d_hoff,
               const uint64_t* d_hsize, uint32_t n, int verify, uint8_t* d_out,
               const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t max_out_cap,
               uint32_t* d_out_len, uint8_t* d_status, uint8_t* scratch, const ReadScratch& R,
               hipStream_t s) {
  uint64_t* dec_in_off = (uint64_t*)(scratch + R.in_off);
  uint32_t* dec_len = (uint32_t*)(scratch + R.len);
  uint64_t* dec_off = (uint64_t*)(scratch + R.off);
  uint32_t* dec_cap = (uint32_t*)(scratch + R.cap);
  uint32_t* dec_olen = (uint32_t*)(scratch + R.olen);
  uint8_t* dec_st = scratch + R.st;
  uint8_t* bad = scratch + R.bad;
  // The dummy slot as an offset from d_out (two's complement wrap).
  const uint64_t dummy_off = (uint64_t)(uintptr_t)(scratch + R.dummy) - (uint64_t)(uintptr_t)d_out;
  // With checksums verified, the CRC pass (verify_kernel) runs on a second
  // stream beside the type dispatch and the decoder, which do not need its
  // result; the merge applies it first, as format.c:203-211 checks the
  // trailer before the type.  Outputs of a block that fails are unspecified.
  hipStream_t a = verify && options().verify_overlap.load() ? aux_stream() : nullptr;
  EventPair ev;
  CheckArgs c{d_file, file_len, d_hoff, d_hsize, verify && !a ? 1u : 0u, d_out, d_out_off, d_out_cap,
              d_out_len, d_status, dec_in_off, dec_len, dec_off, dec_cap, dummy_off, n};
  // (Without verification: one lane per handle; ahead of the verify pass the
  // wave-per-block check, lgs_table.hip.)
  LGS_HIP(verify ? launch_check(c, s) : launch_check_lane(c, s));
  if (a) {
    // After the type dispatch: queued with it, both ran slower (profiles/r6j),
    // and queued first but sleeping through it, its workgroups took the CUs
    // before the decoder's and left some without room for eight decoder
    // waves (365-493 us, profiles/r6r); the event costs ~8 us before the
    // decoder starts (profiles/r6i).
    LGS_HIP(hipEventCreateWithFlags(&ev.e[0], hipEventDisableTiming));
    LGS_HIP(hipEventCreateWithFlags(&ev.e[1], hipEventDisableTiming));
    LGS_HIP(hipEventRecord(ev.e[0], s));
    LGS_HIP(hipStreamWaitEvent(a, ev.e[0], 0));
    LGS_HIP(launch_verify(d_file, file_len, d_hoff, d_hsize, bad, n, a));
    LGS_HIP(hipEventRecord(ev.e[1], a));
  }
  DecodeArgs d{d_file, dec_in_off, dec_len, d_out, dec_off, dec_cap, dec_olen, dec_st, nullptr, n, nullptr};
  LGS_HIP(launch_decode(d, max_out_cap, s));
  if (a) LGS_HIP(hipStreamWaitEvent(s, ev.e[1], 0));
  LGS_HIP(launch_merge(d_status, d_out_len, dec_st, dec_olen, a ? bad : nullptr, n, s));
  return LGS_OK;
}

}  // namespace

size_t lgs_table_write_scratch(uint32_t n, uint64_t raw_total) {
  return WriteScratch(n, raw_total).total;
}

size_t lgs_table_read_scratch(uint32_t n) { return ReadScratch(n).total; }

int lgs_table_write_dev(const uint8_t* d_raw, const uint64_t* d_raw_off,
                        const uint32_t* d_raw_len, uint32_t n, uint32_t max_raw_len,
                        uint64_t raw_total, int compression, uint64_t base, uint8_t* d_file,
                        uint64_t* d_handle_off, uint64_t* d_handle_size, uint64_t* d_end,
                        void* d_scratch, size_t scratch_bytes, void* stream) {
  if (n == 0) return LGS_OK;
  if (!d_raw || !d_raw_off || !d_raw_len || !d_file || !d_handle_off || !d_handle_size ||
      !d_scratch)
    return fail(LGS_EINVAL, "NULL argument");
  if (compression != LGS_NO_COMPRESSION && compression != LGS_SNAPPY_COMPRESSION)
    return fail(LGS_EINVAL, "unknown compression type %d", compression);
  if (max_raw_len > 0x7fffffffu) return fail(LGS_EINVAL, "block of %u bytes too large", max_raw_len);
  const WriteScratch W(n, raw_total);
  if (scratch_bytes < W.total)
    return fail(LGS_EINVAL, "scratch of %zu bytes, %zu needed", scratch_bytes, W.total);
  return table_write(d_raw, d_raw_off, d_raw_len, n, max_raw_len, compression, base, d_file,
                     d_handle_off, d_handle_size, d_end, (uint8_t*)d_scratch, W,
                     (hipStream_t)stream);
}

int lgs_table_read_dev(const uint8_t* d_file, uint64_t file_len, const uint64_t* d_handle_off,
                       const uint64_t* d_handle_size, uint32_t n, int verify_checksums,
                       uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                       uint32_t max_out_cap, uint32_t* d_out_len, uint8_t* d_status,
                       void* d_scratch, size_t scratch_bytes, void* stream) {
  if (n == 0) return LGS_OK;
  if (!d_file || !d_handle_off || !d_handle_size || !d_out || !d_out_off || !d_out_cap ||
      !d_out_len || !d_status || !d_scratch)
    return fail(LGS_EINVAL, "NULL argument");
  const ReadScratch R(n);
  if (scratch_bytes < R.total)
    return fail(LGS_EINVAL, "scratch of %zu bytes, %zu needed", scratch_bytes, R.total);
  return table_read(d_file, file_len, d_handle_off, d_handle_size, n, verify_checksums, d_out,
                    d_out_off, d_out_cap, max_out_cap, d_out_len, d_status, (uint8_t*)d_scratch,
                    R, (hipStream_t)stream);
}

int lgs_table_write_host(const uint8_t* raw, const uint64_t* raw_off, const uint32_t* raw_len,
                         uint32_t n, int compression, uint64_t base, uint8_t* file,
                         size_t file_cap, uint64_t* handle_off, uint64_t* handle_size,
                         uint64_t* end) {
  if (!end) return fail(LGS_EINVAL, "NULL argument");
  if (n == 0) {
    *end = base;
    return LGS_OK;
  }
  if (!raw || !raw_off || !raw_len || !file || !handle_off || !handle_size)
    return fail(LGS_EINVAL, "NULL argument");
  if (compression != LGS_NO_COMPRESSION && compression != LGS_SNAPPY_COMPRESSION)
    return fail(LGS_EINVAL, "unknown compression type %d", compression);
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  size_t in_total = 0;
  uint32_t max_in = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (raw_len[i] > 0x7fffffffu) return fail(LGS_EINVAL, "block %u too large", i);
    in_total += align_up(raw_len[i], 16);
    if (raw_len[i] > max_in) max_in = raw_len[i];
  }
  // Chunks of consecutive blocks are framed independently at file offset 0
  // (a block's framing does not depend on where it lands) and placed at
  // their running offset when they come back.  The staging is two slots,
  // each sized for the largest chunk, used by alternate chunks: the pinned
  // and device arenas stay bounded by the chunk size (LGS_HOST_CHUNK_MB),
  // not by the call, so a multi-GiB table does not pin its whole image.
  const std::vector<uint32_t> first = chunk_bounds(n, in_total, raw_len);
  const uint32_t chunks = (uint32_t)first.size() - 1;
  uint32_t max_n = 0;
  size_t max_inb = 0, max_fo = 0;
  uint64_t max_raw = 0;
  for (uint32_t k = 0; k < chunks; ++k) {
    uint64_t r = 0;
    size_t ib = 0;
    for (uint32_t i = first[k]; i < first[k + 1]; ++i) {
      r += raw_len[i];
      ib += align_up(raw_len[i], 16);
    }
    const uint32_t m = first[k + 1] - first[k];
    const size_t fo = align_up((size_t)r + LGS_TRAILER_SIZE * (size_t)m + 16, 256);
    if (m > max_n) max_n = m;
    if (r > max_raw) max_raw = r;
    if (ib > max_inb) max_inb = ib;
    if (fo > max_fo) max_fo = fo;
  }
  const WriteScratch W(max_n, max_raw + 16 * (uint64_t)max_n);
  Layout L;  // one slot: uploads | downloads | device-only
  const size_t o_in = L.take(max_inb + 16);
  const size_t o_ioff = L.take(8 * (size_t)max_n);
  const size_t o_ilen = L.take(4 * (size_t)max_n);
  const size_t o_hoff = L.take(8 * (size_t)max_n);
  const size_t o_hsize = L.take(8 * (size_t)max_n);
  const size_t o_end = L.take(8);
  const size_t o_file = L.take(max_fo);
  const size_t pin_slot = L.at;
  const size_t o_scr = L.take(W.total);
  const size_t dev_slot = L.at;
  const uint32_t nslot = chunks > 1 ? 2 : 1;
  LGS_TRY(ctx_reserve(c, nslot * dev_slot, nslot * pin_slot));
  uint64_t at = base;                      // file offset of the next chunk
  auto stage = [&](uint32_t k) {
    uint8_t* h = c.h_buf + (k & 1) * pin_slot;
    uint64_t* ioff = (uint64_t*)(h + o_ioff);
    uint32_t* ilen = (uint32_t*)(h + o_ilen);
    size_t ia = o_in;
    for (uint32_t i = first[k]; i < first[k + 1]; ++i) {
      ioff[i - first[k]] = ia;
      ilen[i - first[k]] = raw_len[i];
      ia += align_up(raw_len[i], 16);
    }
    par_for(first[k + 1] - first[k], ia - o_in, [&](uint32_t j0, uint32_t j1) {
      for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t i = first[k] + j;
        memcpy(h + ioff[j], raw + raw_off[i], raw_len[i]);
      }
    });
  };
  auto launch = [&](uint32_t k, hipStream_t s) -> int {
    uint8_t* h = c.h_buf + (k & 1) * pin_slot;
    uint8_t* d = c.d_buf + (k & 1) * dev_slot;
    const uint32_t m = first[k + 1] - first[k];
    const uint64_t* ioff = (const uint64_t*)(h + o_ioff);
    const size_t a1 = ioff[m - 1] + align_up(raw_len[first[k + 1] - 1], 16);
    LGS_HIP(hipMemcpyAsync(d + o_in, h + o_in, a1 - o_in, hipMemcpyHostToDevice, s));
    LGS_HIP(hipMemcpyAsync(d + o_ioff, h + o_ioff, 8 * (size_t)m, hipMemcpyHostToDevice, s));
    LGS_HIP(hipMemcpyAsync(d + o_ilen, h + o_ilen, 4 * (size_t)m, hipMemcpyHostToDevice, s));
    LGS_TRY(table_write(d, (const uint64_t*)(d + o_ioff), (const uint32_t*)(d + o_ilen), m, max_in,
                        compression, 0, d + o_file, (uint64_t*)(d + o_hoff),
                        (uint64_t*)(d + o_hsize), (uint64_t*)(d + o_end), d + o_scr, W, s));
    LGS_HIP(hipMemcpyAsync(h + o_hoff, d + o_hoff, 8 * (size_t)m, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipMemcpyAsync(h + o_hsize, d + o_hsize, 8 * (size_t)m, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipMemcpyAsync(h + o_end, d + o_end, 8, hipMemcpyDeviceToHost, s));
    // The region's size is known only on the device: its bound comes back.
    uint64_t r = 0;
    for (uint32_t i = first[k]; i < first[k + 1]; ++i) r += raw_len[i];
    const size_t fo = align_up((size_t)r + LGS_TRAILER_SIZE * (size_t)m + 16, 256);
    LGS_HIP(hipMemcpyAsync(h + o_file, d + o_file, fo, hipMemcpyDeviceToHost, s));
    return LGS_OK;
  };
  auto finish = [&](uint32_t k) -> int {
    const uint8_t* h = c.h_buf + (k & 1) * pin_slot;
    const uint32_t i0 = first[k], m = first[k + 1] - i0;
    const uint64_t bytes = *(const uint64_t*)(h + o_end);
    if (at - base + bytes > file_cap)
      return fail(LGS_EINVAL, "file buffer of %zu bytes, %zu needed", file_cap,
                  (size_t)(at - base + bytes));
    const uint8_t* src = h + o_file;
    uint8_t* dst = file + (at - base);
    const uint32_t parts = 64;
    const size_t per = ((size_t)bytes + parts - 1) / parts;
    par_for(parts, (size_t)bytes, [&](uint32_t q0, uint32_t q1) {
      const size_t x0 = (size_t)q0 * per, x1 = (size_t)q1 * per < bytes ? (size_t)q1 * per : bytes;
      if (x0 < x1) memcpy(dst + x0, src + x0, x1 - x0);
    });
    const uint64_t* ho = (const uint64_t*)(h + o_hoff);
    const uint64_t* hs = (const uint64_t*)(h + o_hsize);
    for (uint32_t j = 0; j < m; ++j) {
      handle_off[i0 + j] = ho[j] + at;
      handle_size[i0 + j] = hs[j];
    }
    at += bytes;
    return LGS_OK;
  };
  LGS_TRY(pipeline(c, chunks, stage, launch, finish));
  *end = at;
  return LGS_OK;
}

int lgs_table_read_host(const uint8_t* file, uint64_t file_len, const uint64_t* handle_off,
                        const uint64_t* handle_size, uint32_t n, int verify_checksums,
                        uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                        uint32_t* out_len, uint8_t* status) {
  if (n == 0) return LGS_OK;
  if (!file || !handle_off || !handle_size || !out || !out_off || !out_cap || !out_len || !status)
    return fail(LGS_EINVAL, "NULL argument");
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  // Only each block's byte range (+ trailer) travels, packed 16-aligned into
  // its chunk's image; a range outside the file keeps an offset past that
  // image, so the device reports the truncated read itself (format.c:195-198).
  auto in_file = [&](uint32_t i) {
    const uint64_t o = handle_off[i], sz = handle_size[i];
    return sz <= ~0ull - LGS_TRAILER_SIZE && o <= file_len && file_len - o >= sz + LGS_TRAILER_SIZE;
  };
  size_t out_total = 0;
  uint32_t max_cap = 0;
  for (uint32_t i = 0; i < n; ++i) {
    out_total += align_up(out_cap[i], 16);
    if (out_cap[i] > max_cap) max_cap = out_cap[i];
  }
  // Chunks of consecutive handles through the two-stream pipeline (see
  // pipeline()), staged in two slots sized for the largest chunk (bounded
  // by LGS_HOST_CHUNK_MB, not by the call; see lgs_table_write_host).
  const std::vector<uint32_t> first = chunk_bounds(n, out_total, out_cap);
  const uint32_t chunks = (uint32_t)first.size() - 1;
  uint32_t max_n = 0;
  size_t max_blk = 0, max_out = 0;
  for (uint32_t k = 0; k < chunks; ++k) {
    size_t bb = 0, ob = 0;
    for (uint32_t i = first[k]; i < first[k + 1]; ++i) {
      if (in_file(i)) bb += align_up((size_t)handle_size[i] + LGS_TRAILER_SIZE, 16);
      ob += align_up(out_cap[i], 16);
    }
    if (first[k + 1] - first[k] > max_n) max_n = first[k + 1] - first[k];
    if (bb > max_blk) max_blk = bb;
    if (ob > max_out) max_out = ob;
  }
  const ReadScratch R(max_n);
  Layout L;  // one slot
  const size_t o_blk = L.take(max_blk + 16);
  const size_t o_hoff = L.take(8 * (size_t)max_n);
  const size_t o_hsize = L.take(8 * (size_t)max_n);
  const size_t o_ooff = L.take(8 * (size_t)max_n);
  const size_t o_ocap = L.take(4 * (size_t)max_n);
  const size_t o_st = L.take((size_t)max_n);
  const size_t o_olen = L.take(4 * (size_t)max_n);
  const size_t o_out = L.take(max_out + 16);
  const size_t pin_slot = L.at;
  const size_t o_scr = L.take(R.total);
  const size_t dev_slot = L.at;
  const uint32_t nslot = chunks > 1 ? 2 : 1;
  LGS_TRY(ctx_reserve(c, nslot * dev_slot, nslot * pin_slot));
  std::vector<size_t> blk_len(chunks, 0);   // each chunk's packed image length
  auto stage = [&](uint32_t k) {
    uint8_t* h = c.h_buf + (k & 1) * pin_slot;
    uint64_t* hoff = (uint64_t*)(h + o_hoff);
    uint64_t* hsize = (uint64_t*)(h + o_hsize);
    uint64_t* ooff = (uint64_t*)(h + o_ooff);
    uint32_t* ocap = (uint32_t*)(h + o_ocap);
    size_t ba = 0, oa = o_out;
    const uint32_t i0 = first[k], m = first[k + 1] - i0;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t i = i0 + j;
      hsize[j] = handle_size[i];
      hoff[j] = in_file(i) ? ba : ~0ull;
      if (in_file(i)) ba += align_up((size_t)handle_size[i] + LGS_TRAILER_SIZE, 16);
      ooff[j] = oa;
      ocap[j] = out_cap[i];
      oa += align_up(out_cap[i], 16);
    }
    blk_len[k] = ba;
    for (uint32_t j = 0; j < m; ++j)
      if (hoff[j] == ~0ull) hoff[j] = ba + 16 + 1;   // past the image: a truncated read
    par_for(m, ba, [&](uint32_t j0, uint32_t j1) {
      for (uint32_t j = j0; j < j1; ++j)
        if (hoff[j] <= ba)
          memcpy(h + o_blk + hoff[j], file + handle_off[i0 + j], (size_t)hsize[j] + LGS_TRAILER_SIZE);
    });
  };
  auto launch = [&](uint32_t k, hipStream_t s) -> int {
    uint8_t* h = c.h_buf + (k & 1) * pin_slot;
    uint8_t* d = c.d_buf + (k & 1) * dev_slot;
    const uint32_t m = first[k + 1] - first[k];
    const uint64_t* ooff = (const uint64_t*)(h + o_ooff);
    if (blk_len[k] > 0)
      LGS_HIP(hipMemcpyAsync(d + o_blk, h + o_blk, blk_len[k], hipMemcpyHostToDevice, s));
    for (const size_t o : {o_hoff, o_hsize, o_ooff})
      LGS_HIP(hipMemcpyAsync(d + o, h + o, 8 * (size_t)m, hipMemcpyHostToDevice, s));
    LGS_HIP(hipMemcpyAsync(d + o_ocap, h + o_ocap, 4 * (size_t)m, hipMemcpyHostToDevice, s));
    LGS_TRY(table_read(d + o_blk, blk_len[k] + 16, (const uint64_t*)(d + o_hoff),
                       (const uint64_t*)(d + o_hsize), m, verify_checksums, d,
                       (const uint64_t*)(d + o_ooff), (const uint32_t*)(d + o_ocap), max_cap,
                       (uint32_t*)(d + o_olen), d + o_st, d + o_scr, R, s));
    LGS_HIP(hipMemcpyAsync(h + o_st, d + o_st, m, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipMemcpyAsync(h + o_olen, d + o_olen, 4 * (size_t)m, hipMemcpyDeviceToHost, s));
    const size_t oe = ooff[m - 1] + align_up(out_cap[first[k + 1] - 1], 16);
    LGS_HIP(hipMemcpyAsync(h + o_out, d + o_out, oe - o_out, hipMemcpyDeviceToHost, s));
    return LGS_OK;
  };
  auto finish = [&](uint32_t k) -> int {
    const uint8_t* h = c.h_buf + (k & 1) * pin_slot;
    const uint32_t i0 = first[k], m = first[k + 1] - i0;
    const uint32_t* olen = (const uint32_t*)(h + o_olen);
    const uint64_t* ooff = (const uint64_t*)(h + o_ooff);
    const size_t bytes = ooff[m - 1] + out_cap[first[k + 1] - 1] - ooff[0];
    par_for(m, bytes, [&](uint32_t j0, uint32_t j1) {
      for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t i = i0 + j;
        status[i] = h[o_st + j];
        out_len[i] = olen[j];
        if (status[i] == LGS_ST_OK) memcpy(out + out_off[i], h + ooff[j], olen[j]);
      }
    });
    return LGS_OK;
  };
  LGS_TRY(pipeline(c, chunks, stage, launch, finish));
  return LGS_OK;
}

// ---- bloom filter (kernels: lgs_bloom.hip) ----

namespace {

static uint32_t bloom_k(int bpk) {                        // bloom.c:35-45
  size_t k = (size_t)(bpk * 0.69);
  if (k < 1) k = 1;
  if (k > 30) k = 30;
  return (uint32_t)k;
}

static size_t bloom_bytes(uint64_t n, int bpk) {          // bloom.c:69-80
  uint64_t bits = n * (uint64_t)bpk;
  if (bits < 64) bits = 64;
  return (size_t)((bits + 7) / 8);
}

constexpr int kMaxBitsPerKey = 1 << 16;

}  // namespace

size_t lgs_bloom_filter_size(uint32_t nkeys, int bits_per_key) {
  if (nkeys == 0 || bits_per_key < 0) return 0;
  return bloom_bytes(nkeys, bits_per_key) + 1;
}

int lgs_bloom_build_dev(const uint8_t* d_keys, const uint64_t* d_key_off,
                        const uint32_t* d_key_len, const uint32_t* d_first, uint32_t nfilters,
                        int bits_per_key, uint8_t* d_out, const uint64_t* d_out_off,
                        void* stream) {
  if (nfilters == 0) return LGS_OK;
  if (!d_keys || !d_key_off || !d_key_len || !d_first || !d_out || !d_out_off)
    return fail(LGS_EINVAL, "NULL argument");
  if (bits_per_key < 0 || bits_per_key > kMaxBitsPerKey)
    return fail(LGS_EINVAL, "bits_per_key %d out of range", bits_per_key);
  LGS_HIP(launch_bloom_build(d_keys, d_key_off, d_key_len, d_first, nfilters,
                             (uint32_t)bits_per_key, bloom_k(bits_per_key), d_out, d_out_off,
                             0, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_bloom_match_dev(const uint8_t* d_filters, const uint64_t* d_filter_off,
                        const uint32_t* d_filter_len, const uint32_t* d_query_filter,
                        const uint8_t* d_keys, const uint64_t* d_key_off,
                        const uint32_t* d_key_len, uint8_t* d_match, uint32_t nq, void* stream) {
  if (nq == 0) return LGS_OK;
  if (!d_filters || !d_filter_off || !d_filter_len || !d_query_filter || !d_keys || !d_key_off ||
      !d_key_len || !d_match)
    return fail(LGS_EINVAL, "NULL argument");
  LGS_HIP(launch_bloom_match(d_filters, d_filter_off, d_filter_len, d_query_filter, d_keys,
                             d_key_off, d_key_len, d_match, nq, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_bloom_build_host(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len,
                         const uint32_t* first, uint32_t nfilters, int bits_per_key,
                         uint8_t* out, const uint64_t* out_off) {
  if (nfilters == 0) return LGS_OK;
  if (!keys || !key_off || !key_len || !first || !out || !out_off)
    return fail(LGS_EINVAL, "NULL argument");
  if (bits_per_key < 0 || bits_per_key > kMaxBitsPerKey)
    return fail(LGS_EINVAL, "bits_per_key %d out of range", bits_per_key);
  for (uint32_t f = 0; f < nfilters; ++f)
    if (first[f + 1] < first[f]) return fail(LGS_EINVAL, "first[] decreases at filter %u", f);
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  const uint32_t nkeys = first[nfilters] - first[0];
  const uint32_t k0 = first[0];
  size_t key_bytes = 0, filt_bytes = 0;
  for (uint32_t i = k0; i < k0 + nkeys; ++i) key_bytes += key_len[i];
  for (uint32_t f = 0; f < nfilters; ++f)
    filt_bytes += lgs_bloom_filter_size(first[f + 1] - first[f], bits_per_key);
  Layout L;  // upload | download
  const size_t o_keys = L.take(key_bytes + 16);
  const size_t o_koff = L.take(8 * (size_t)nkeys);
  const size_t o_klen = L.take(4 * (size_t)nkeys);
  const size_t o_first = L.take(4 * ((size_t)nfilters + 1));
  const size_t o_foff = L.take(8 * (size_t)nfilters);
  const size_t up_end = L.at;
  const size_t o_filt = L.take(filt_bytes + 16);
  const size_t down_end = L.at;
  LGS_TRY(ctx_reserve(c, down_end, down_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  uint64_t* koff = (uint64_t*)(h + o_koff);
  uint32_t* klen = (uint32_t*)(h + o_klen);
  uint32_t* fst = (uint32_t*)(h + o_first);
  uint64_t* foff = (uint64_t*)(h + o_foff);
  size_t at = o_keys;
  for (uint32_t j = 0; j < nkeys; ++j) {
    memcpy(h + at, keys + key_off[k0 + j], key_len[k0 + j]);
    koff[j] = at;
    klen[j] = key_len[k0 + j];
    at += key_len[k0 + j];
  }
  memset(h + at, 0, 16);
  size_t fat = 0;
  for (uint32_t f = 0; f <= nfilters; ++f) fst[f] = first[f] - k0;
  for (uint32_t f = 0; f < nfilters; ++f) {
    foff[f] = fat;
    fat += lgs_bloom_filter_size(first[f + 1] - first[f], bits_per_key);
  }
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, c.stream));
  LGS_HIP(launch_bloom_build(d, (const uint64_t*)(d + o_koff), (const uint32_t*)(d + o_klen),
                             (const uint32_t*)(d + o_first), nfilters, (uint32_t)bits_per_key,
                             bloom_k(bits_per_key), d + o_filt, (const uint64_t*)(d + o_foff),
                             0, c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_filt, d + o_filt, filt_bytes, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  for (uint32_t f = 0; f < nfilters; ++f)
    memcpy(out + out_off[f], h + o_filt + foff[f],
           lgs_bloom_filter_size(first[f + 1] - first[f], bits_per_key));
  return LGS_OK;
}

int lgs_bloom_match_host(const uint8_t* filters, const uint64_t* filter_off,
                         const uint32_t* filter_len, uint32_t nfilters,
                         const uint32_t* query_filter, const uint8_t* keys,
                         const uint64_t* key_off, const uint32_t* key_len, uint32_t nq,
                         uint8_t* match) {
  if (nq == 0) return LGS_OK;
  if (!filters || !filter_off || !filter_len || !query_filter || !keys || !key_off || !key_len ||
      !match)
    return fail(LGS_EINVAL, "NULL argument");
  for (uint32_t q = 0; q < nq; ++q)
    if (query_filter[q] >= nfilters)
      return fail(LGS_EINVAL, "query %u names filter %u of %u", q, query_filter[q], nfilters);
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  size_t fb = 0, kb = 0;
  for (uint32_t f = 0; f < nfilters; ++f) fb += filter_len[f];
  for (uint32_t q = 0; q < nq; ++q) kb += key_len[q];
  Layout L;
  const size_t o_f = L.take(fb + 16);
  const size_t o_foff = L.take(8 * (size_t)nfilters);
  const size_t o_flen = L.take(4 * (size_t)nfilters);
  const size_t o_qf = L.take(4 * (size_t)nq);
  const size_t o_k = L.take(kb + 16);
  const size_t o_koff = L.take(8 * (size_t)nq);
  const size_t o_klen = L.take(4 * (size_t)nq);
  const size_t up_end = L.at;
  const size_t o_m = L.take(nq);
  const size_t down_end = L.at;
  LGS_TRY(ctx_reserve(c, down_end, down_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  uint64_t* foff = (uint64_t*)(h + o_foff);
  uint32_t* flen = (uint32_t*)(h + o_flen);
  uint64_t* koff = (uint64_t*)(h + o_koff);
  uint32_t* klen = (uint32_t*)(h + o_klen);
  size_t at = 0;
  for (uint32_t f = 0; f < nfilters; ++f) {
    memcpy(h + o_f + at, filters + filter_off[f], filter_len[f]);
    foff[f] = at;
    flen[f] = filter_len[f];
    at += filter_len[f];
  }
  memset(h + o_f + at, 0, 16);
  memcpy(h + o_qf, query_filter, 4 * (size_t)nq);
  at = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    memcpy(h + o_k + at, keys + key_off[q], key_len[q]);
    koff[q] = at;
    klen[q] = key_len[q];
    at += key_len[q];
  }
  memset(h + o_k + at, 0, 16);
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, c.stream));
  LGS_HIP(launch_bloom_match(d + o_f, (const uint64_t*)(d + o_foff), (const uint32_t*)(d + o_flen),
                             (const uint32_t*)(d + o_qf), d + o_k, (const uint64_t*)(d + o_koff),
                             (const uint32_t*)(d + o_klen), d + o_m, nq, c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_m, d + o_m, nq, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  memcpy(match, h + o_m, nq);
  return LGS_OK;
}

// ---- the filter block (filter_block.c; kernels: lgs_bloom.hip) ----

namespace {

constexpr uint64_t kMaxDataEnd = 1ull << 42;   // 2^31 filters: offsets fit the u32 array

struct FilterScratch {
  size_t kf, foff, part, meta, total;
  explicit FilterScratch(uint64_t data_end) {
    const size_t nf = (size_t)(data_end >> 11) + 2;
    Layout L;
    kf = L.take(4 * nf);
    foff = L.take(8 * nf);
    part = L.take(8 * filter_block_parts(data_end));
    meta = L.take(12);
    total = L.at;
  }
};

static int filter_args(uint32_t nblocks, uint64_t data_end, int bits_per_key, int internal_keys) {
  if (bits_per_key < 0 || bits_per_key > kMaxBitsPerKey)
    return fail(LGS_EINVAL, "bits_per_key %d out of range", bits_per_key);
  if (data_end >= kMaxDataEnd) return fail(LGS_EINVAL, "data_end %llu too large",
                                           (unsigned long long)data_end);
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  (void)nblocks;
  return LGS_OK;
}

}  // namespace

size_t lgs_filter_block_bound(uint32_t nkeys, uint32_t nblocks, uint64_t data_end,
                              int bits_per_key) {
  if (bits_per_key < 0 || data_end >= kMaxDataEnd) return 0;
  // Nonempty filters <= nblocks, each <= n * bpk / 8 + 10 bytes; 4 bytes per
  // filter offset (<= data_end / 2048 + 1 of them), 5 trailing.
  return (size_t)(((uint64_t)nkeys * (uint64_t)bits_per_key + 7) / 8 + 10ull * nblocks +
                  4ull * ((data_end >> 11) + 1) + 5);
}

size_t lgs_filter_block_scratch(uint64_t data_end) {
  if (data_end >= kMaxDataEnd) return 0;
  return FilterScratch(data_end).total;
}

int lgs_filter_block_build_dev(const uint8_t* d_keys, const uint64_t* d_key_off,
                               const uint32_t* d_key_len, uint32_t nkeys,
                               const uint32_t* d_block_first, const uint64_t* d_block_off,
                               uint32_t nblocks, uint64_t data_end, int bits_per_key,
                               int internal_keys, uint8_t* d_out, size_t out_cap,
                               uint64_t* d_size, void* d_scratch, size_t scratch_bytes,
                               void* stream) {
  LGS_TRY(filter_args(nblocks, data_end, bits_per_key, internal_keys));
  if (!d_block_first || !d_out || !d_size || !d_scratch || (nblocks && !d_block_off) ||
      (nkeys && (!d_keys || !d_key_off || !d_key_len)))
    return fail(LGS_EINVAL, "NULL argument");
  const FilterScratch S(data_end);
  if (scratch_bytes < S.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_filter_block_scratch)", scratch_bytes,
                S.total);
  const size_t bound = lgs_filter_block_bound(nkeys, nblocks, data_end, bits_per_key);
  if (out_cap < bound)
    return fail(LGS_ENOSPC, "out_cap %zu < %zu (lgs_filter_block_bound)", out_cap, bound);
  uint8_t* sc = (uint8_t*)d_scratch;
  LGS_HIP(launch_filter_block_build(d_keys, d_key_off, d_key_len, d_block_first, d_block_off,
                                    nblocks, data_end, (uint32_t)bits_per_key,
                                    bloom_k(bits_per_key), internal_keys ? 8u : 0u, d_out,
                                    d_size, (uint32_t*)(sc + S.kf), (uint64_t*)(sc + S.foff),
                                    (uint64_t*)(sc + S.part), (uint32_t*)(sc + S.meta),
                                    (hipStream_t)stream));
  return LGS_OK;
}

int lgs_filter_block_build_host(const uint8_t* keys, const uint64_t* key_off,
                                const uint32_t* key_len, const uint32_t* block_first,
                                const uint64_t* block_off, uint32_t nblocks, uint64_t data_end,
                                int bits_per_key, int internal_keys, uint8_t* out,
                                size_t out_cap, size_t* size) {
  LGS_TRY(filter_args(nblocks, data_end, bits_per_key, internal_keys));
  if (!block_first || !out || !size || (nblocks && !block_off))
    return fail(LGS_EINVAL, "NULL argument");
  for (uint32_t b = 0; b < nblocks; ++b) {
    if (block_first[b + 1] < block_first[b])
      return fail(LGS_EINVAL, "block_first[] decreases at block %u", b);
    if ((b + 1 < nblocks ? block_off[b + 1] : data_end) < block_off[b])
      return fail(LGS_EINVAL, "block offsets decrease at block %u", b);
  }
  const uint32_t k0 = block_first[0], nkeys = block_first[nblocks] - k0;
  if (nkeys && (!keys || !key_off || !key_len)) return fail(LGS_EINVAL, "NULL argument");
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  size_t key_bytes = 0;
  for (uint32_t i = k0; i < k0 + nkeys; ++i) key_bytes += key_len[i];
  const size_t bound = lgs_filter_block_bound(nkeys, nblocks, data_end, bits_per_key);
  const FilterScratch S(data_end);
  Layout L;  // upload | scratch | download
  const size_t o_keys = L.take(key_bytes + 16);
  const size_t o_koff = L.take(8 * (size_t)nkeys);
  const size_t o_klen = L.take(4 * (size_t)nkeys);
  const size_t o_bf = L.take(4 * ((size_t)nblocks + 1));
  const size_t o_bo = L.take(8 * (size_t)nblocks);
  const size_t up_end = L.at;
  const size_t o_scr = L.take(S.total);
  const size_t o_size = L.take(8);
  const size_t o_out = L.take(bound);
  const size_t down_end = o_out + bound;
  LGS_TRY(ctx_reserve(c, L.at, L.at));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  uint64_t* koff = (uint64_t*)(h + o_koff);
  uint32_t* klen = (uint32_t*)(h + o_klen);
  uint32_t* bf = (uint32_t*)(h + o_bf);
  size_t at = o_keys;
  for (uint32_t j = 0; j < nkeys; ++j) {
    memcpy(h + at, keys + key_off[k0 + j], key_len[k0 + j]);
    koff[j] = at;
    klen[j] = key_len[k0 + j];
    at += key_len[k0 + j];
  }
  memset(h + at, 0, 16);
  for (uint32_t b = 0; b <= nblocks; ++b) bf[b] = block_first[b] - k0;
  if (nblocks) memcpy(h + o_bo, block_off, 8 * (size_t)nblocks);
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, c.stream));
  LGS_TRY(lgs_filter_block_build_dev(d, (const uint64_t*)(d + o_koff),
                                     (const uint32_t*)(d + o_klen), nkeys,
                                     (const uint32_t*)(d + o_bf), (const uint64_t*)(d + o_bo),
                                     nblocks, data_end, bits_per_key, internal_keys, d + o_out,
                                     bound, (uint64_t*)(d + o_size), d + o_scr, S.total,
                                     c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_size, d + o_size, down_end - o_size, hipMemcpyDeviceToHost,
                         c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  const uint64_t n = *(const uint64_t*)(h + o_size);
  if (n > bound) return fail(LGS_EINTERNAL, "filter block %llu > bound %zu",
                             (unsigned long long)n, bound);
  *size = (size_t)n;
  if (n > out_cap) return fail(LGS_ENOSPC, "filter block needs %llu bytes, out_cap %zu",
                               (unsigned long long)n, out_cap);
  memcpy(out, h + o_out, (size_t)n);
  return LGS_OK;
}

int lgs_filter_block_match_dev(const uint8_t* d_block, size_t block_len,
                               const uint64_t* d_block_offset, const uint8_t* d_keys,
                               const uint64_t* d_key_off, const uint32_t* d_key_len, uint32_t nq,
                               int internal_keys, uint8_t* d_match, void* stream) {
  if (nq == 0) return LGS_OK;
  if ((block_len && !d_block) || !d_block_offset || !d_keys || !d_key_off || !d_key_len ||
      !d_match)
    return fail(LGS_EINVAL, "NULL argument");
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  LGS_HIP(launch_filter_block_match(d_block, block_len, d_block_offset, d_keys, d_key_off,
                                    d_key_len, internal_keys ? 8u : 0u, d_match, nq,
                                    (hipStream_t)stream));
  return LGS_OK;
}

int lgs_filter_block_match_host(const uint8_t* block, size_t block_len,
                                const uint64_t* block_offset, const uint8_t* keys,
                                const uint64_t* key_off, const uint32_t* key_len, uint32_t nq,
                                int internal_keys, uint8_t* match) {
  if (nq == 0) return LGS_OK;
  if ((block_len && !block) || !block_offset || !keys || !key_off || !key_len || !match)
    return fail(LGS_EINVAL, "NULL argument");
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  size_t kb = 0;
  for (uint32_t q = 0; q < nq; ++q) kb += key_len[q];
  Layout L;
  const size_t o_b = L.take(block_len + 16);
  const size_t o_qo = L.take(8 * (size_t)nq);
  const size_t o_k = L.take(kb + 16);
  const size_t o_koff = L.take(8 * (size_t)nq);
  const size_t o_klen = L.take(4 * (size_t)nq);
  const size_t up_end = L.at;
  const size_t o_m = L.take(nq);
  LGS_TRY(ctx_reserve(c, L.at, L.at));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  if (block_len) memcpy(h + o_b, block, block_len);
  memcpy(h + o_qo, block_offset, 8 * (size_t)nq);
  uint64_t* koff = (uint64_t*)(h + o_koff);
  uint32_t* klen = (uint32_t*)(h + o_klen);
  size_t at = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    memcpy(h + o_k + at, keys + key_off[q], key_len[q]);
    koff[q] = at;
    klen[q] = key_len[q];
    at += key_len[q];
  }
  memset(h + o_k + at, 0, 16);
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, c.stream));
  LGS_TRY(lgs_filter_block_match_dev(d + o_b, block_len, (const uint64_t*)(d + o_qo), d + o_k,
                                     (const uint64_t*)(d + o_koff),
                                     (const uint32_t*)(d + o_klen), nq, internal_keys, d + o_m,
                                     c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_m, d + o_m, nq, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  memcpy(match, h + o_m, nq);
  return LGS_OK;
}

// ---- the data-block builder and whole tables (kernels: lgs_block.hip) ----

namespace {

constexpr uint32_t kMaxEntries = 0x7fffffffu;
constexpr uint64_t kMaxEntryBytes = 1ull << 30;   // key + value of one entry
const char kFilterName[] = "filter.leveldb.BuiltinBloomFilter2";   // "filter." + bloom.c's name

// The builder's device scratch (BlockScratch, lgs_launch.h).
struct BlockBuildScratch {
  size_t lcp, sh, S, ca, cb, next, ja, jb, mark, bid, icut, ilen, part, total;
  explicit BlockBuildScratch(uint32_t n) {
    const size_t m = (size_t)n + 1;
    Layout L;
    lcp = L.take(4 * m);
    sh = L.take(4 * m);
    S = L.take(8 * m);
    ca = L.take(8 * m);
    cb = L.take(8 * m);
    next = L.take(4 * m);
    ja = L.take(4 * m);
    jb = L.take(4 * m);
    mark = L.take(4 * m);
    bid = L.take(8 * m);
    icut = L.take(4 * m);
    ilen = L.take(4 * m);
    part = L.take(8 * scan_parts(n) + 8);
    total = L.at;
  }
  BlockScratch at(uint8_t* p) const {
    return BlockScratch{(uint32_t*)(p + lcp), (uint32_t*)(p + sh), (uint64_t*)(p + S),
                        (uint64_t*)(p + ca), (uint64_t*)(p + cb), (uint32_t*)(p + next),
                        (uint32_t*)(p + ja), (uint32_t*)(p + jb), (uint32_t*)(p + mark),
                        (uint64_t*)(p + bid), (uint32_t*)(p + icut), (uint32_t*)(p + ilen),
                        (uint64_t*)(p + part)};
  }
};

static int block_args(uint32_t n, uint32_t restart_interval, int internal_keys) {
  if (n > kMaxEntries) return fail(LGS_EINVAL, "%u entries: at most 2^31 - 1", n);
  if (restart_interval == 0) return fail(LGS_EINVAL, "restart_interval must be at least 1");
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  return LGS_OK;
}

// Host entries staged key after key and value after value (uploads of one
// _host call), and the checks a _dev caller vouches for.
struct EntryStage {
  size_t keys, vals, koff, klen, voff, vlen;
  uint64_t kb = 0, vb = 0;
};

static int entries_check(const uint32_t* key_len, const uint32_t* val_len, uint32_t n,
                         int internal_keys, EntryStage* E) {
  for (uint32_t i = 0; i < n; ++i) {
    if ((uint64_t)key_len[i] + val_len[i] >= kMaxEntryBytes)
      return fail(LGS_EINVAL, "entry %u: key + value of %llu bytes, under 2^30 supported", i,
                  (unsigned long long)key_len[i] + val_len[i]);
    if (internal_keys && key_len[i] < 8)
      return fail(LGS_EINVAL, "entry %u: internal key of %u bytes (at least 8)", i, key_len[i]);
    E->kb += key_len[i];
    E->vb += val_len[i];
  }
  return LGS_OK;
}

static void entries_layout(Layout& L, uint32_t n, EntryStage* E) {
  E->keys = L.take((size_t)E->kb + 16);
  E->vals = L.take((size_t)E->vb + 16);
  E->koff = L.take(8 * (size_t)n);
  E->klen = L.take(4 * (size_t)n);
  E->voff = L.take(8 * (size_t)n);
  E->vlen = L.take(4 * (size_t)n);
}

static void entries_stage(uint8_t* h, const EntryStage& E, const uint8_t* keys,
                          const uint64_t* key_off, const uint32_t* key_len, const uint8_t* vals,
                          const uint64_t* val_off, const uint32_t* val_len, uint32_t n) {
  uint64_t* koff = (uint64_t*)(h + E.koff);
  uint64_t* voff = (uint64_t*)(h + E.voff);
  uint64_t ka = 0, va = 0;
  for (uint32_t i = 0; i < n; ++i) {
    koff[i] = ka;
    voff[i] = va;
    ka += key_len[i];
    va += val_len[i];
  }
  memcpy(h + E.klen, key_len, 4 * (size_t)n);
  memcpy(h + E.vlen, val_len, 4 * (size_t)n);
  par_for(n, (size_t)(ka + va), [&](uint32_t i0, uint32_t i1) {
    for (uint32_t i = i0; i < i1; ++i) {
      memcpy(h + E.keys + koff[i], keys + key_off[i], key_len[i]);
      memcpy(h + E.vals + voff[i], vals + val_off[i], val_len[i]);
    }
  });
  memset(h + E.keys + ka, 0, 16);
  memset(h + E.vals + va, 0, 16);
}

static BlockIn entries_in(uint8_t* d, const EntryStage& E, uint32_t n) {
  return BlockIn{d + E.keys, (const uint64_t*)(d + E.koff), (const uint32_t*)(d + E.klen),
                 d + E.vals, (const uint64_t*)(d + E.voff), (const uint32_t*)(d + E.vlen), n};
}

// The cut's outputs inside an arena.
struct CutLayout {
  size_t bf, roff, rlen, ioff;
  void take(Layout& L, uint32_t n) {
    bf = L.take(4 * ((size_t)n + 1));
    roff = L.take(8 * ((size_t)n + 1));
    rlen = L.take(4 * ((size_t)n + 1));
    ioff = L.take(8 * ((size_t)n + 1));
  }
  BlockCut at(uint8_t* p, uint64_t* counts) const {
    return BlockCut{(uint32_t*)(p + bf), (uint64_t*)(p + roff), (uint32_t*)(p + rlen),
                    (uint64_t*)(p + ioff), counts};
  }
};

// Index block bound: one block of n entries (restart interval 1) whose keys
// total key_bytes and whose values are handles of at most 20 bytes.
static size_t index_block_bound(uint32_t n, uint64_t key_bytes) {
  return (size_t)(key_bytes + (20ull + 7 + 4) * n + 8);
}

}  // namespace

size_t lgs_block_build_bound(uint32_t n, uint64_t key_bytes, uint64_t value_bytes) {
  // Every entry a block of its own: an 11-byte header at most, one restart
  // and the restart count; 16 readable bytes after the last block.
  return (size_t)(key_bytes + value_bytes + 19ull * n + 16);
}

size_t lgs_block_build_scratch(uint32_t n) { return BlockBuildScratch(n).total; }

size_t lgs_table_build_bound(uint32_t n, uint64_t key_bytes, uint64_t value_bytes,
                             int bits_per_key) {
  const uint64_t data = key_bytes + value_bytes + 19ull * n + (uint64_t)LGS_TRAILER_SIZE * n;
  const uint64_t filter =
      bits_per_key > 0 ? lgs_filter_block_bound(n, n, data, bits_per_key) + LGS_TRAILER_SIZE : 0;
  return (size_t)(data + filter + kMetaindexMax + LGS_TRAILER_SIZE + index_block_bound(n, key_bytes) +
                  LGS_TRAILER_SIZE + kFooterSize);
}

int lgs_block_cut_dev(const uint8_t* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
                      const uint32_t* d_val_len, uint32_t n, uint64_t block_size,
                      uint32_t restart_interval, int internal_keys, uint32_t* d_block_first,
                      uint64_t* d_raw_off, uint32_t* d_raw_len, uint64_t* d_ikey_off,
                      uint64_t* d_counts, void* d_scratch, size_t scratch_bytes, void* stream) {
  LGS_TRY(block_args(n, restart_interval, internal_keys));
  if (!d_block_first || !d_raw_off || !d_raw_len || !d_ikey_off || !d_counts || !d_scratch ||
      (n && (!d_keys || !d_key_off || !d_key_len || !d_val_len)))
    return fail(LGS_EINVAL, "NULL argument");
  const BlockBuildScratch B(n);
  if (scratch_bytes < B.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_block_build_scratch)", scratch_bytes, B.total);
  const BlockIn in{d_keys, d_key_off, d_key_len, nullptr, nullptr, d_val_len, n};
  const BlockCut out{d_block_first, d_raw_off, d_raw_len, d_ikey_off, d_counts};
  LGS_HIP(launch_block_cut(in, block_size, restart_interval, internal_keys ? 8u : 0u,
                           B.at((uint8_t*)d_scratch), out, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_block_emit_dev(const uint8_t* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
                       const uint8_t* d_vals, const uint64_t* d_val_off, const uint32_t* d_val_len,
                       uint32_t n, uint32_t restart_interval, int internal_keys, uint32_t nblocks,
                       const uint32_t* d_block_first, const uint64_t* d_raw_off,
                       const uint32_t* d_raw_len, uint8_t* d_raw, const uint64_t* d_ikey_off,
                       uint8_t* d_ikey, void* d_scratch, size_t scratch_bytes, void* stream) {
  LGS_TRY(block_args(n, restart_interval, internal_keys));
  if (nblocks > n) return fail(LGS_EINVAL, "%u blocks of %u entries", nblocks, n);
  if (n == 0) return LGS_OK;
  if (!d_keys || !d_key_off || !d_key_len || !d_vals || !d_val_off || !d_val_len ||
      !d_block_first || !d_raw_off || !d_raw_len || !d_raw || !d_scratch || (d_ikey && !d_ikey_off))
    return fail(LGS_EINVAL, "NULL argument");
  const BlockBuildScratch B(n);
  if (scratch_bytes < B.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_block_build_scratch)", scratch_bytes, B.total);
  const BlockIn in{d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, n};
  LGS_HIP(launch_block_emit(in, restart_interval, internal_keys ? 8u : 0u, nblocks,
                            B.at((uint8_t*)d_scratch), d_block_first, d_raw_off, d_raw_len, d_raw,
                            d_ikey_off, d_ikey, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_block_build_host(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len,
                         const uint8_t* vals, const uint64_t* val_off, const uint32_t* val_len,
                         uint32_t n, uint64_t block_size, uint32_t restart_interval,
                         int internal_keys, uint8_t* raw, size_t raw_cap, uint64_t* raw_off,
                         uint32_t* raw_len, uint32_t* block_first, uint8_t* ikey, size_t ikey_cap,
                         uint64_t* ikey_off, uint32_t* nblocks) {
  LGS_TRY(block_args(n, restart_interval, internal_keys));
  if (!raw_off || !raw_len || !block_first || !ikey_off || !nblocks ||
      (n && (!keys || !key_off || !key_len || !vals || !val_off || !val_len || !raw || !ikey)))
    return fail(LGS_EINVAL, "NULL argument");
  EntryStage E;
  LGS_TRY(entries_check(key_len, val_len, n, internal_keys, &E));
  *nblocks = 0;
  block_first[0] = 0;
  raw_off[0] = 0;
  ikey_off[0] = 0;
  if (n == 0) return LGS_OK;
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  const size_t bound = lgs_block_build_bound(n, E.kb, E.vb);
  const BlockBuildScratch B(n);
  Layout L;  // uploads | downloads | device-only
  entries_layout(L, n, &E);
  const size_t up_end = L.at;
  const size_t o_cnt = L.take(8 * kBlockCounts);
  CutLayout K;
  K.take(L, n);
  const size_t o_raw = L.take(bound);
  const size_t o_ikey = L.take((size_t)E.kb + 16);
  const size_t pin_end = L.at;
  const size_t o_scr = L.take(B.total);
  LGS_TRY(ctx_reserve(c, L.at, pin_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  entries_stage(h, E, keys, key_off, key_len, vals, val_off, val_len, n);
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, c.stream));
  const BlockIn in = entries_in(d, E, n);
  const BlockCut cut = K.at(d, (uint64_t*)(d + o_cnt));
  const uint32_t trim = internal_keys ? 8u : 0u;
  LGS_HIP(launch_block_cut(in, block_size, restart_interval, trim, B.at(d + o_scr), cut, c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_cnt, d + o_cnt, 8 * kBlockCounts, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  const uint64_t* cnt = (const uint64_t*)(h + o_cnt);
  const uint64_t nb = cnt[0], raw_total = cnt[1], ikey_total = cnt[3];
  if (nb > n || raw_total + 16 > bound || ikey_total > E.kb)
    return fail(LGS_EINTERNAL, "cut of %u entries: %llu blocks, %llu + %llu bytes", n,
                (unsigned long long)nb, (unsigned long long)raw_total,
                (unsigned long long)ikey_total);
  if (cnt[2] > 0x7fffffffull)
    return fail(LGS_EINVAL, "a block of %llu bytes: under 2^31 supported",
                (unsigned long long)cnt[2]);
  if (raw_total > raw_cap || ikey_total > ikey_cap)
    return fail(LGS_ENOSPC, "blocks need %llu bytes (raw_cap %zu), index keys %llu (ikey_cap %zu)",
                (unsigned long long)raw_total, raw_cap, (unsigned long long)ikey_total, ikey_cap);
  LGS_HIP(launch_block_emit(in, restart_interval, trim, (uint32_t)nb, B.at(d + o_scr),
                            cut.block_first, cut.raw_off, cut.raw_len, d + o_raw, cut.ikey_off,
                            d + o_ikey, c.stream));
  LGS_HIP(hipMemcpyAsync(h + K.bf, d + K.bf, o_raw - K.bf, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_raw, d + o_raw, (size_t)raw_total, hipMemcpyDeviceToHost, c.stream));
  LGS_HIP(hipMemcpyAsync(h + o_ikey, d + o_ikey, (size_t)ikey_total, hipMemcpyDeviceToHost,
                         c.stream));
  LGS_HIP(hipStreamSynchronize(c.stream));
  memcpy(block_first, h + K.bf, 4 * ((size_t)nb + 1));
  memcpy(raw_off, h + K.roff, 8 * ((size_t)nb + 1));
  memcpy(raw_len, h + K.rlen, 4 * (size_t)nb);
  memcpy(ikey_off, h + K.ioff, 8 * ((size_t)nb + 1));
  memcpy(raw, h + o_raw, (size_t)raw_total);
  memcpy(ikey, h + o_ikey, (size_t)ikey_total);
  *nblocks = (uint32_t)nb;
  return LGS_OK;
}

int lgs_table_build_host(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len,
                         const uint8_t* vals, const uint64_t* val_off, const uint32_t* val_len,
                         uint32_t n, uint64_t block_size, uint32_t restart_interval,
                         int compression, int bits_per_key, int internal_keys, uint8_t* file,
                         size_t file_cap, size_t* file_size) {
  LGS_TRY(block_args(n, restart_interval, internal_keys));
  if (compression != LGS_NO_COMPRESSION && compression != LGS_SNAPPY_COMPRESSION)
    return fail(LGS_EINVAL, "unknown compression type %d", compression);
  if (bits_per_key < 0 || bits_per_key > kMaxBitsPerKey)
    return fail(LGS_EINVAL, "bits_per_key %d out of range", bits_per_key);
  if (!file || !file_size || (n && (!keys || !key_off || !key_len || !vals || !val_off || !val_len)))
    return fail(LGS_EINVAL, "NULL argument");
  EntryStage E;
  LGS_TRY(entries_check(key_len, val_len, n, internal_keys, &E));
  // The smallest table: two 8-byte blocks with trailers and the footer.
  if (file_cap < 2 * (8 + LGS_TRAILER_SIZE) + kFooterSize)
    return fail(LGS_ENOSPC, "file_cap %zu: no table fits", file_cap);
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  const uint32_t trim = internal_keys ? 8u : 0u;
  const bool filter = bits_per_key > 0;
  const size_t raw_bound = lgs_block_build_bound(n, E.kb, E.vb);
  const uint64_t data_bound = raw_bound + (uint64_t)LGS_TRAILER_SIZE * n;
  if (data_bound >= kMaxDataEnd) return fail(LGS_EINVAL, "table of %llu bytes too large",
                                             (unsigned long long)data_bound);
  const size_t fbound = filter ? lgs_filter_block_bound(n, n, data_bound, bits_per_key) : 0;
  const size_t ibound = index_block_bound(n, E.kb);
  if (fbound > 0x7fffffffull || ibound > 0x7fffffffull)
    return fail(LGS_EINVAL, "filter or index block over 2^31 bytes");
  const size_t img_bound = lgs_table_build_bound(n, E.kb, E.vb, bits_per_key);
  const BlockBuildScratch B(n);
  const FilterScratch F(data_bound);
  size_t wtotal = WriteScratch(n, raw_bound).total;
  if (WriteScratch(1, fbound).total > wtotal) wtotal = WriteScratch(1, fbound).total;
  Layout L;  // uploads | small downloads | device-only
  entries_layout(L, n, &E);
  const size_t up_end = L.at;
  const size_t o_meta = L.take(kMetaindexMax + 16);   // tail uploads: metaindex, {offset, length} x 2
  const size_t o_toff = L.take(16);
  const size_t o_tlen = L.take(8);
  const size_t o_tencoff = L.take(16);
  // The tail's encoder items: the metaindex block and the index block's 64 KiB
  // chunks ({input offset, output slot} u64, {length, header} u32 each).
  const uint32_t icap = 2 + (uint32_t)(ibound / kChunk);
  const size_t o_titems = L.take(24 * (size_t)icap);
  const size_t o_cnt = L.take(8 * kBlockCounts);      // downloads
  const size_t o_cnt2 = L.take(8 * kBlockCounts);
  const size_t o_end = L.take(8);
  const size_t o_fsize = L.take(8);
  const size_t o_thoff = L.take(16);
  const size_t o_thsize = L.take(16);
  const size_t pin_end = L.at;
  CutLayout K, K2;
  K.take(L, n);
  K2.take(L, n);
  const size_t o_raw = L.take(raw_bound);
  const size_t o_ikey = L.take((size_t)E.kb + 16);
  const size_t o_scr = L.take(B.total);
  const size_t o_wscr = L.take(wtotal);
  const size_t o_hoff = L.take(8 * (size_t)n + 8);
  const size_t o_hsize = L.take(8 * (size_t)n + 8);
  const size_t o_fscr = L.take(F.total);
  const size_t o_fout = L.take(fbound + 16);
  const size_t o_hval = L.take(20 * (size_t)n + 16);
  const size_t o_ivoff = L.take(8 * (size_t)n + 8);
  const size_t o_ivlen = L.take(4 * (size_t)n + 4);
  const size_t o_iklen = L.take(4 * (size_t)n + 4);
  const size_t o_iraw = L.take(ibound + 16);
  const size_t o_file = L.take(img_bound + 16);
  const size_t o_tslots = L.take((size_t)icap * chunk_out(kChunk));
  const size_t o_tpacked = L.take(bound_of(ibound) + 64);
  const size_t o_tenclen = L.take(4 * (size_t)icap);
  const size_t o_tenclen2 = L.take(8);
  const size_t o_tpoff = L.take(8 * (size_t)icap);
  const size_t o_tptotal = L.take(8);
  const size_t o_tfoff = L.take(16);
  const size_t o_tpart = L.take(8 * scan_parts(icap) + 16);
  LGS_TRY(ctx_reserve(c, L.at, pin_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  hipStream_t s = c.stream;
  uint64_t nb = 0, raw_total = 0, max_raw = 0;
  const BlockIn in = entries_in(d, E, n);
  const BlockCut cut = K.at(d, (uint64_t*)(d + o_cnt));
  if (n) {
    entries_stage(h, E, keys, key_off, key_len, vals, val_off, val_len, n);
    LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, s));
    LGS_HIP(launch_block_cut(in, block_size, restart_interval, trim, B.at(d + o_scr), cut, s));
    LGS_HIP(hipMemcpyAsync(h + o_cnt, d + o_cnt, 8 * kBlockCounts, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    const uint64_t* cnt = (const uint64_t*)(h + o_cnt);
    nb = cnt[0], raw_total = cnt[1], max_raw = cnt[2];
    if (nb == 0 || nb > n || raw_total + 16 > raw_bound || cnt[3] > E.kb)
      return fail(LGS_EINTERNAL, "cut of %u entries: %llu blocks, %llu bytes", n,
                  (unsigned long long)nb, (unsigned long long)raw_total);
    if (max_raw > 0x7fffffffull)
      return fail(LGS_EINVAL, "a block of %llu bytes: under 2^31 supported",
                  (unsigned long long)max_raw);
  } else {
    LGS_HIP(hipMemsetAsync(d + K.bf, 0, 4, s));
  }
  // Data blocks (table_builder.c:215-278), framed from file offset 0.
  uint64_t* d_hoff = (uint64_t*)(d + o_hoff);
  uint64_t* d_hsize = (uint64_t*)(d + o_hsize);
  uint64_t data_end = 0;
  const BlockCut cut2 = K2.at(d, (uint64_t*)(d + o_cnt2));
  const BlockIn iin{d + o_ikey, cut.ikey_off, (const uint32_t*)(d + o_iklen), d + o_hval,
                    (const uint64_t*)(d + o_ivoff), (const uint32_t*)(d + o_ivlen), (uint32_t)nb};
  uint64_t index_len = 0;
  if (nb) {
    LGS_HIP(launch_block_emit(in, restart_interval, trim, (uint32_t)nb, B.at(d + o_scr),
                              cut.block_first, cut.raw_off, cut.raw_len, d + o_raw, cut.ikey_off,
                              d + o_ikey, s));
    LGS_TRY(table_write(d + o_raw, cut.raw_off, cut.raw_len, (uint32_t)nb, (uint32_t)max_raw,
                        compression, 0, d + o_file, d_hoff, d_hsize, (uint64_t*)(d + o_end),
                        d + o_wscr, WriteScratch((uint32_t)nb, raw_total), s));
    // The index block's entries (:229-239, :332-341): index key -> handle, one
    // block whatever its size, restart interval 1 (:87).
    LGS_HIP(launch_handle_values(d_hoff, d_hsize, cut.ikey_off, (uint32_t)nb, d + o_hval,
                                 (uint64_t*)(d + o_ivoff), (uint32_t*)(d + o_ivlen),
                                 (uint32_t*)(d + o_iklen), s));
    LGS_HIP(launch_block_cut(iin, ~0ull, 1, 0, B.at(d + o_scr), cut2, s));
    LGS_HIP(hipMemcpyAsync(h + o_cnt2, d + o_cnt2, 8 * kBlockCounts, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipMemcpyAsync(h + o_end, d + o_end, 8, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    data_end = *(const uint64_t*)(h + o_end);
    const uint64_t* cnt2 = (const uint64_t*)(h + o_cnt2);
    index_len = cnt2[1];
    if (data_end > data_bound || cnt2[0] != 1 || index_len > ibound)
      return fail(LGS_EINTERNAL, "data blocks end at %llu, index block of %llu bytes",
                  (unsigned long long)data_end, (unsigned long long)index_len);
    LGS_HIP(launch_block_emit(iin, 1, 0, 1, B.at(d + o_scr), cut2.block_first, cut2.raw_off,
                              cut2.raw_len, d + o_iraw, nullptr, nullptr, s));
  } else {
    // An index block with no entries (block_builder.c:68, :143-146).
    index_len = tail_metaindex(h + o_meta, kMetaindexMax, nullptr, 0, 0);
    LGS_HIP(hipMemcpyAsync(d + o_iraw, h + o_meta, (size_t)index_len, hipMemcpyHostToDevice, s));
    LGS_HIP(hipStreamSynchronize(s));
  }
  // The filter block (:292-299), stored raw after the data blocks.
  uint64_t at = data_end, filter_size = 0;
  if (filter) {
    LGS_TRY(lgs_filter_block_build_dev(in.keys, in.key_off, in.key_len, n, cut.block_first, d_hoff,
                                       (uint32_t)nb, data_end, bits_per_key, internal_keys,
                                       d + o_fout, fbound, (uint64_t*)(d + o_fsize), d + o_fscr,
                                       F.total, s));
    LGS_HIP(hipMemcpyAsync(h + o_fsize, d + o_fsize, 8, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    filter_size = *(const uint64_t*)(h + o_fsize);
    if (filter_size > fbound)
      return fail(LGS_EINTERNAL, "filter block %llu > bound %zu", (unsigned long long)filter_size,
                  fbound);
    *(uint64_t*)(h + o_toff) = 0;
    *(uint32_t*)(h + o_tlen) = (uint32_t)filter_size;
    LGS_HIP(hipMemcpyAsync(d + o_toff, h + o_toff, 8, hipMemcpyHostToDevice, s));
    LGS_HIP(hipMemcpyAsync(d + o_tlen, h + o_tlen, 4, hipMemcpyHostToDevice, s));
    LGS_TRY(table_write(d + o_fout, (const uint64_t*)(d + o_toff), (const uint32_t*)(d + o_tlen), 1,
                        (uint32_t)filter_size, LGS_NO_COMPRESSION, at, d + o_file + at,
                        (uint64_t*)(d + o_thoff), (uint64_t*)(d + o_thsize), nullptr, d + o_wscr,
                        WriteScratch(1, filter_size), s));
    // The pinned words are reused below: the uploads must have left them.
    LGS_HIP(hipStreamSynchronize(s));
    at += filter_size + LGS_TRAILER_SIZE;
  }
  // Metaindex (:301-328) and index (:330-344) blocks, both through the
  // table's compression like every block ldb_tablegen_write_block writes.
  // The index block grows with the table (C5: 36 MB), and one block is one
  // wave's work in the encoder, 64 KiB chunk after chunk; the chunks are
  // independent (snappy.c:370-381), so they are encoded here as items of
  // their own, as ldb_snappy_encode does, and packed into the block's stream.
  const size_t meta_len = tail_metaindex(h + o_meta, kMetaindexMax, filter ? kFilterName : nullptr,
                                         data_end, filter_size);
  if (meta_len == 0) return fail(LGS_EINTERNAL, "metaindex block does not fit");
  const bool snappy = compression == LGS_SNAPPY_COMPRESSION;
  uint64_t* toff = (uint64_t*)(h + o_toff);
  uint32_t* tlen = (uint32_t*)(h + o_tlen);
  uint64_t* tenc_off = (uint64_t*)(h + o_tencoff);
  toff[0] = o_meta;          // offsets from the arena's start
  toff[1] = o_iraw;
  tlen[0] = (uint32_t)meta_len;
  tlen[1] = (uint32_t)index_len;
  tenc_off[0] = o_tslots;
  tenc_off[1] = o_tpacked;
  const uint32_t items = 1 + (uint32_t)((index_len + kChunk - 1) / kChunk);
  if (items > icap) return fail(LGS_EINTERNAL, "index block of %llu bytes",
                                (unsigned long long)index_len);
  uint64_t* it_in = (uint64_t*)(h + o_titems);
  uint64_t* it_out = it_in + icap;
  uint32_t* it_len = (uint32_t*)(it_out + icap);
  uint32_t* it_hdr = it_len + icap;
  it_in[0] = o_meta;
  it_len[0] = it_hdr[0] = (uint32_t)meta_len;
  it_out[0] = o_tslots;
  size_t slot = o_tslots + chunk_out((uint32_t)meta_len);
  for (uint32_t j = 1; j < items; ++j) {
    const uint64_t off = (uint64_t)(j - 1) * kChunk;
    it_in[j] = o_iraw + off;
    it_len[j] = (uint32_t)(index_len - off < kChunk ? index_len - off : kChunk);
    it_hdr[j] = j == 1 ? (uint32_t)index_len : 0xffffffffu;      // snappy.c:368
    it_out[j] = slot;
    slot += chunk_out(it_len[j]);
  }
  LGS_HIP(hipMemcpyAsync(d + o_meta, h + o_meta, o_cnt - o_meta, hipMemcpyHostToDevice, s));
  uint64_t* part = (uint64_t*)(d + o_tpart);
  uint32_t* enc_len = (uint32_t*)(d + o_tenclen);
  uint32_t* enc_len2 = (uint32_t*)(d + o_tenclen2);
  if (snappy) {
    const uint64_t* d_out = (const uint64_t*)(d + o_titems) + icap;
    const uint32_t* d_len = (const uint32_t*)(d_out + icap);
    EncodeArgs ea{d, (const uint64_t*)(d + o_titems), d_len, d, d_out, enc_len, d_len + icap,
                  nullptr, items, nullptr};
    const uint32_t ichunk = (uint32_t)(index_len < kChunk ? index_len : kChunk);
    LGS_HIP(launch_encode(ea, meta_len > ichunk ? (uint32_t)meta_len : ichunk, s));
    LGS_HIP(launch_scan(2, nullptr, enc_len + 1, part, 0, (uint64_t*)(d + o_tpoff),
                        (uint64_t*)(d + o_tptotal), items - 1, s));
    LGS_HIP(launch_pack(d, d_out + 1, enc_len + 1, d + o_tpacked, (const uint64_t*)(d + o_tpoff),
                        items - 1, s));
    LGS_HIP(launch_pair_lens(enc_len, (const uint64_t*)(d + o_tptotal), enc_len2, s));
  }
  LGS_HIP(launch_scan(1, (const uint32_t*)(d + o_tlen), snappy ? enc_len2 : nullptr, part, at,
                      (uint64_t*)(d + o_tfoff), (uint64_t*)(d + o_end), 2, s));
  const FrameArgs fa{d, (const uint64_t*)(d + o_toff), (const uint32_t*)(d + o_tlen), d,
                     (const uint64_t*)(d + o_tencoff), snappy ? enc_len2 : nullptr,
                     d + o_file + at, at, (const uint64_t*)(d + o_tfoff),
                     (uint64_t*)(d + o_thoff), (uint64_t*)(d + o_thsize), 2};
  LGS_HIP(launch_frame(fa, s));
  LGS_HIP(hipMemcpyAsync(h + o_end, d + o_end, pin_end - o_end, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  const uint64_t end = *(const uint64_t*)(h + o_end);
  const uint64_t* thoff = (const uint64_t*)(h + o_thoff);
  const uint64_t* thsize = (const uint64_t*)(h + o_thsize);
  if (end > img_bound)
    return fail(LGS_EINTERNAL, "table of %llu bytes > bound %zu", (unsigned long long)end, img_bound);
  *file_size = (size_t)(end + kFooterSize);
  if (end + kFooterSize > file_cap)
    return fail(LGS_ENOSPC, "table needs %llu bytes, file_cap %zu",
                (unsigned long long)(end + kFooterSize), file_cap);
  LGS_HIP(hipMemcpyAsync(file, d + o_file, (size_t)end, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  tail_footer(file + end, thoff[0], thsize[0], thoff[1], thsize[1]);   // :346-362
  return LGS_OK;
}

// ---- batched point lookups (kernels: lgs_seek.hip) ----

size_t lgs_block_seek_scratch(uint32_t nq) { return align_up(4 * (size_t)nq, 256); }

int lgs_block_seek_dev(const uint8_t* d_blocks, const uint64_t* d_block_off,
                       const uint32_t* d_block_len, const uint8_t* d_block_status,
                       uint32_t nblocks, const uint32_t* d_query_block, const uint8_t* d_keys,
                       const uint64_t* d_key_off, const uint32_t* d_key_len, uint32_t nq,
                       int internal_keys, uint32_t* d_entry_pos, uint32_t* d_found_key_len,
                       uint32_t* d_val_pos, uint32_t* d_val_len, uint8_t* d_status,
                       uint8_t* d_key_out, const uint64_t* d_key_out_off,
                       const uint32_t* d_key_out_cap, void* d_scratch, size_t scratch_bytes,
                       void* stream) {
  if (nq == 0) return LGS_OK;
  if ((nblocks && (!d_blocks || !d_block_off || !d_block_len)) || !d_query_block || !d_keys ||
      !d_key_off || !d_key_len || !d_entry_pos || !d_found_key_len || !d_val_pos || !d_val_len ||
      !d_status || !d_scratch || (d_key_out && (!d_key_out_off || !d_key_out_cap)))
    return fail(LGS_EINVAL, "NULL argument");
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  if (scratch_bytes < lgs_block_seek_scratch(nq))
    return fail(LGS_EINVAL, "scratch of %zu bytes, %zu needed", scratch_bytes,
                lgs_block_seek_scratch(nq));
  const SeekArgs a{d_blocks, d_block_off, d_block_len, d_block_status, nblocks, d_query_block,
                   d_keys, d_key_off, d_key_len, nq, (uint32_t)internal_keys, d_entry_pos,
                   d_found_key_len, d_val_pos, d_val_len, d_status, (uint32_t*)d_scratch,
                   d_key_out, d_key_out_off, d_key_out_cap};
  LGS_HIP(launch_block_seek(a, (hipStream_t)stream));
  return LGS_OK;
}

namespace {

// What the read path needs to know of one block handle before the launch:
// whether its bytes and trailer lie inside the file, and the room its
// contents take (the raw size, or a Snappy block's size header,
// snappy.c:386-399).  A header beyond anything `size` bytes of Snappy can
// expand to (64 bytes per 3-byte copy) cannot decode: the room is capped
// there and the decoder's LGS_ST_NOSPACE stands for the reference's
// "corrupted compressed block contents" (format.c:247-251).
struct HandlePlan {
  bool in_file = false;
  uint32_t cap = 0;
};

int plan_handle(const uint8_t* file, uint64_t file_len, uint64_t off, uint64_t size,
                HandlePlan* p) {
  p->in_file = size <= ~0ull - LGS_TRAILER_SIZE && off <= file_len &&
               file_len - off >= size + LGS_TRAILER_SIZE;
  p->cap = 0;
  if (!p->in_file) return LGS_OK;
  if (size > 0x7fffffffull)
    return fail(LGS_EINVAL, "a block of %llu bytes: under 2^31 supported", (unsigned long long)size);
  p->cap = (uint32_t)size;
  if (file[off + size] == LGS_SNAPPY_COMPRESSION) {
    uint32_t want = 0;
    const uint64_t most = 32 * size + 64;
    p->cap = read_varint32(&want, file + off, (size_t)size) ? want : 0;
    if (p->cap > most) p->cap = (uint32_t)most;
  }
  return LGS_OK;
}

struct HandleKey {
  uint64_t off, size;
  bool operator==(const HandleKey& o) const { return off == o.off && size == o.size; }
};
struct HandleHash {
  size_t operator()(const HandleKey& k) const {
    return (size_t)((k.off * 0x9e3779b97f4a7c15ull) ^ (k.size + (k.off >> 32)));
  }
};

// Stages n handles for table_read: their byte ranges packed 16-aligned at
// h_blk (lgs_table_read_host's layout: a handle outside the file points past
// the image, so the device reports the truncated read), the handle arrays
// and each block's 16-aligned output slot from out_base on.  Returns the
// image's length; *out_end = the end of the slots.
size_t stage_handles(const uint8_t* file, const uint64_t* off, const uint64_t* size,
                     const HandlePlan* plan, uint32_t n, uint8_t* h_blk, uint64_t* hoff,
                     uint64_t* hsize, uint64_t* ooff, uint32_t* ocap, size_t out_base,
                     size_t* out_end) {
  size_t ba = 0, oa = out_base;
  for (uint32_t j = 0; j < n; ++j) {
    hsize[j] = size[j];
    hoff[j] = plan[j].in_file ? ba : ~0ull;
    if (plan[j].in_file) ba += align_up((size_t)size[j] + LGS_TRAILER_SIZE, 16);
    ooff[j] = oa;
    ocap[j] = plan[j].cap;
    oa += align_up(plan[j].cap, 16);
  }
  for (uint32_t j = 0; j < n; ++j)
    if (hoff[j] == ~0ull) hoff[j] = ba + 16 + 1;
  par_for(n, ba, [&](uint32_t j0, uint32_t j1) {
    for (uint32_t j = j0; j < j1; ++j)
      if (hoff[j] <= ba) memcpy(h_blk + hoff[j], file + off[j], (size_t)size[j] + LGS_TRAILER_SIZE);
  });
  *out_end = oa;
  return ba;
}

size_t handles_image(const uint64_t* size, const HandlePlan* plan, uint32_t n, size_t* out_bytes,
                     uint32_t* max_cap) {
  size_t ba = 0, oa = 0;
  uint32_t mc = 0;
  for (uint32_t j = 0; j < n; ++j) {
    if (plan[j].in_file) ba += align_up((size_t)size[j] + LGS_TRAILER_SIZE, 16);
    oa += align_up(plan[j].cap, 16);
    if (plan[j].cap > mc) mc = plan[j].cap;
  }
  *out_bytes = oa;
  *max_cap = mc;
  return ba;
}

}  // namespace

int lgs_table_get_host(const uint8_t* file, uint64_t file_len, int verify_checksums,
                       int paranoid_checks, int internal_keys, const char* filter_name,
                       const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len,
                       uint32_t nq, uint8_t* called, uint8_t* status, uint8_t* verdict,
                       uint8_t* out, size_t out_cap, uint64_t* out_key_off,
                       uint64_t* out_val_off, size_t* out_needed) {
  if (!file || !out_needed || !out_key_off || !out_val_off)
    return fail(LGS_EINVAL, "NULL argument");
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  *out_needed = 0;
  out_key_off[0] = out_val_off[0] = 0;
  if (nq == 0) return LGS_OK;
  if (!keys || !key_off || !key_len || !called || !status || (out_cap && !out))
    return fail(LGS_EINVAL, "NULL argument");
  if (nq > kMaxEntries) return fail(LGS_EINVAL, "%u queries: under 2^31 supported", nq);
  size_t kb = 0;
  for (uint32_t q = 0; q < nq; ++q) kb += key_len[q];
  // ldb_table_open on the host: footer and metaindex (before the lease: the
  // metaindex read takes a context of its own).
  uint64_t h2_off[2] = {0, 0}, h2_size[2] = {0, 0};
  uint8_t open_st = LGS_ST_OK;
  LGS_TRY(table_open(file, file_len, paranoid_checks, filter_name, &h2_off[0], &h2_size[0],
                     &h2_off[1], &h2_size[1], &open_st));
  auto all_fail = [&](uint8_t st) {
    for (uint32_t q = 0; q < nq; ++q) {
      called[q] = 0;
      status[q] = st;
      if (verdict) verdict[q] = kGetNotFound;
      out_key_off[q + 1] = out_val_off[q + 1] = 0;
    }
    return LGS_OK;
  };
  if (open_st != LGS_ST_OK) return all_fail(open_st);
  const bool want_filter = h2_off[1] != ~0ull;
  const uint32_t n2 = want_filter ? 2u : 1u;
  HandlePlan plan2[2];
  for (uint32_t j = 0; j < n2; ++j)
    LGS_TRY(plan_handle(file, file_len, h2_off[j], h2_size[j], &plan2[j]));
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  hipStream_t s = c.stream;

  // -- A: index (and filter) block, the index seek, the handles, the filter.
  size_t out2 = 0;
  uint32_t max_cap2 = 0;
  const size_t img2 = handles_image(h2_size, plan2, n2, &out2, &max_cap2);
  const ReadScratch R2(n2);
  Layout L;  // uploads | downloads | device-only
  const size_t o_keys = L.take(kb + 16);
  const size_t o_koff = L.take(8 * (size_t)nq);
  const size_t o_klen = L.take(4 * (size_t)nq);
  const size_t o_blk = L.take(img2 + 32);
  const size_t o_hoff = L.take(16);
  const size_t o_hsize = L.take(16);
  const size_t o_ooff = L.take(16);
  const size_t o_ocap = L.take(8);
  const size_t o_zero = L.take(8);
  const size_t up_end = L.at;
  const size_t o_state = L.take(nq);           // downloads, contiguous
  const size_t o_match = L.take(nq);
  const size_t o_sst = L.take(nq);
  const size_t o_qhoff = L.take(8 * (size_t)nq);
  const size_t o_qhsize = L.take(8 * (size_t)nq);
  const size_t o_bst = L.take(2);
  const size_t down_end = L.at;
  const size_t o_olen = L.take(8);
  const size_t o_epos = L.take(4 * (size_t)nq);
  const size_t o_fkl = L.take(4 * (size_t)nq);
  const size_t o_vpos = L.take(4 * (size_t)nq);
  const size_t o_vlen = L.take(4 * (size_t)nq);
  const size_t o_rpos = L.take(lgs_block_seek_scratch(nq));
  const size_t o_rscr = L.take(R2.total);
  const size_t o_out2 = L.take(out2 + 16);
  LGS_TRY(ctx_reserve(c, L.at, down_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  {
    uint64_t* koff = (uint64_t*)(h + o_koff);
    uint32_t* klen = (uint32_t*)(h + o_klen);
    size_t at = 0;
    for (uint32_t q = 0; q < nq; ++q) {
      koff[q] = at;
      klen[q] = key_len[q];
      at += key_len[q];
    }
    par_for(nq, kb, [&](uint32_t q0, uint32_t q1) {
      for (uint32_t q = q0; q < q1; ++q) memcpy(h + o_keys + koff[q], keys + key_off[q], key_len[q]);
    });
    memset(h + o_keys + kb, 0, 16);
    *(uint64_t*)(h + o_zero) = 0;
  }
  size_t out2_end = 0;
  stage_handles(file, h2_off, h2_size, plan2, n2, h + o_blk, (uint64_t*)(h + o_hoff),
                (uint64_t*)(h + o_hsize), (uint64_t*)(h + o_ooff), (uint32_t*)(h + o_ocap), o_out2,
                &out2_end);
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, s));
  const uint8_t* d_keys = d + o_keys;
  const uint64_t* d_koff = (const uint64_t*)(d + o_koff);
  const uint32_t* d_klen = (const uint32_t*)(d + o_klen);
  uint32_t* d_epos = (uint32_t*)(d + o_epos);
  uint32_t* d_fkl = (uint32_t*)(d + o_fkl);
  uint32_t* d_vpos = (uint32_t*)(d + o_vpos);
  uint32_t* d_vlen = (uint32_t*)(d + o_vlen);
  uint32_t* d_rpos = (uint32_t*)(d + o_rpos);
  LGS_TRY(table_read(d + o_blk, img2 + 16, (const uint64_t*)(d + o_hoff),
                     (const uint64_t*)(d + o_hsize), n2, paranoid_checks, d,
                     (const uint64_t*)(d + o_ooff), (const uint32_t*)(d + o_ocap), max_cap2,
                     (uint32_t*)(d + o_olen), d + o_bst, d + o_rscr, R2, s));
  // The index block stays where the read put it: block 0 of the seek.
  const SeekArgs ia{d + o_out2, (const uint64_t*)(d + o_zero), (const uint32_t*)(d + o_olen),
                    d + o_bst, 1, nullptr, d_keys, d_koff, d_klen, nq, (uint32_t)internal_keys,
                    d_epos, d_fkl, d_vpos, d_vlen, d + o_sst, d_rpos, nullptr, nullptr, nullptr};
  LGS_HIP(launch_block_seek(ia, s));
  LGS_HIP(launch_get_handles(d + o_out2, d_epos, d_vpos, d_vlen, nq, (uint64_t*)(d + o_qhoff),
                             (uint64_t*)(d + o_qhsize), d + o_state, s));
  if (want_filter) {
    // The block's length as the host knows it; a filter block that does not
    // read is dropped below (table.c:71-72), whatever was matched in it.
    const size_t f_at = o_out2 + align_up(plan2[0].cap, 16);
    LGS_HIP(launch_filter_block_match(d + f_at, plan2[1].cap, (const uint64_t*)(d + o_qhoff), d_keys,
                                      d_koff, d_klen, internal_keys ? 8u : 0u, d + o_match, nq, s));
  }
  LGS_HIP(hipMemcpyAsync(h + o_state, d + o_state, down_end - o_state, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));   // the read-back that sizes and de-duplicates the block read

  // -- B: the distinct data blocks the surviving queries name.
  const bool filter = want_filter && h[o_bst + 1] == LGS_ST_OK;
  std::vector<uint32_t> qblock(nq, kNoBlock);
  std::vector<uint8_t> pre(nq, LGS_ST_OK);
  std::vector<uint64_t> b_off, b_size;
  {
    const uint8_t* state = h + o_state;
    const uint8_t* match = h + o_match;
    const uint8_t* sst = h + o_sst;
    const uint64_t* qho = (const uint64_t*)(h + o_qhoff);
    const uint64_t* qhs = (const uint64_t*)(h + o_qhsize);
    std::unordered_map<HandleKey, uint32_t, HandleHash> seen;
    for (uint32_t q = 0; q < nq; ++q) {
      if (state[q] == 0) {
        pre[q] = sst[q];                                   // the index iterator's status
      } else if (state[q] == 2) {
        pre[q] = LGS_ST_CORRUPT;                           // table.c:244-245
      } else if (!filter || match[q]) {
        const HandleKey k{qho[q], qhs[q]};
        auto it = seen.find(k);
        if (it == seen.end()) {
          it = seen.emplace(k, (uint32_t)b_off.size()).first;
          b_off.push_back(k.off);
          b_size.push_back(k.size);
        }
        qblock[q] = it->second;
      }
    }
  }
  const uint32_t nb = (uint32_t)b_off.size();
  std::vector<HandlePlan> plan(nb);
  for (uint32_t j = 0; j < nb; ++j)
    LGS_TRY(plan_handle(file, file_len, b_off[j], b_size[j], &plan[j]));
  size_t outb = 0;
  uint32_t max_cap = 0;
  const size_t img = handles_image(b_size.data(), plan.data(), nb, &outb, &max_cap);
  const ReadScratch R(nb);
  Layout B;  // uploads | downloads | device-only
  const size_t p_blk = B.take(img + 32);
  const size_t p_hoff = B.take(8 * (size_t)nb);
  const size_t p_hsize = B.take(8 * (size_t)nb);
  const size_t p_ooff = B.take(8 * (size_t)nb);
  const size_t p_ocap = B.take(4 * (size_t)nb);
  const size_t p_qblock = B.take(4 * (size_t)nq);
  const size_t p_pre = B.take(nq);
  const size_t pin_b = B.at;
  const size_t p_koff = B.take(8 * ((size_t)nq + 1));
  const size_t p_voff = B.take(8 * ((size_t)nq + 1));
  const size_t p_called = B.take(nq);
  const size_t p_fst = B.take(nq);
  const size_t p_verdict = B.take(nq);
  const size_t p_olen = B.take(4 * (size_t)nb);
  const size_t p_bst = B.take(nb);
  const size_t p_len = B.take(4 * (size_t)nq);
  const size_t p_sst = B.take(nq);
  const size_t p_vsrc = B.take(8 * (size_t)nq);
  const size_t p_vn = B.take(4 * (size_t)nq);
  const size_t p_part = B.take(8 * scan_parts(nq) + 8);
  const size_t p_rscr = B.take(R.total);
  const size_t p_out = B.take(outb + 16);
  LGS_TRY(ctx_reserve(c, 0, pin_b));
  h = c.h_buf;
  Scratch arena(B.at, s);
  if (arena.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%zu bytes of device memory for %u blocks: %s", B.at, nb,
                hipGetErrorString(arena.status()));
  uint8_t* e = (uint8_t*)arena.get();
  size_t outb_end = 0;
  stage_handles(file, b_off.data(), b_size.data(), plan.data(), nb, h + p_blk,
                (uint64_t*)(h + p_hoff), (uint64_t*)(h + p_hsize), (uint64_t*)(h + p_ooff),
                (uint32_t*)(h + p_ocap), p_out, &outb_end);
  memcpy(h + p_qblock, qblock.data(), 4 * (size_t)nq);
  memcpy(h + p_pre, pre.data(), nq);
  LGS_HIP(hipMemcpyAsync(e, h, pin_b, hipMemcpyHostToDevice, s));
  if (nb)
    LGS_TRY(table_read(e + p_blk, img + 16, (const uint64_t*)(e + p_hoff),
                       (const uint64_t*)(e + p_hsize), nb, verify_checksums, e,
                       (const uint64_t*)(e + p_ooff), (const uint32_t*)(e + p_ocap), max_cap,
                       (uint32_t*)(e + p_olen), e + p_bst, e + p_rscr, R, s));
  const uint32_t* d_qblock = (const uint32_t*)(e + p_qblock);
  const SeekArgs da{e, (const uint64_t*)(e + p_ooff), (const uint32_t*)(e + p_olen), e + p_bst, nb,
                    d_qblock, d_keys, d_koff, d_klen, nq, (uint32_t)internal_keys, d_epos, d_fkl,
                    d_vpos, d_vlen, e + p_sst, d_rpos, nullptr, nullptr, nullptr};
  LGS_HIP(launch_block_seek(da, s));
  LGS_HIP(launch_get_lens(d_qblock, e + p_pre, d_epos, d_fkl, d_vlen, e + p_sst, nq, e + p_called,
                          e + p_fst, (uint32_t*)(e + p_len), s));
  uint64_t* d_okoff = (uint64_t*)(e + p_koff);
  LGS_HIP(launch_scan(2, nullptr, (const uint32_t*)(e + p_len), (uint64_t*)(e + p_part), 0, d_okoff,
                      d_okoff + nq, nq, s));
  LGS_HIP(hipMemcpyAsync(out_key_off, d_okoff, 8 * ((size_t)nq + 1), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(called, e + p_called, nq, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(status, e + p_fst, nq, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  for (uint32_t q = 0; q < nq; ++q)
    if (status[q] == LGS_ST_NOSPACE) status[q] = LGS_ST_CORRUPT;   // plan_handle's cap
  const uint64_t total = out_key_off[nq];
  *out_needed = (size_t)total;
  if (total > out_cap)
    return fail(LGS_ENOSPC, "results take %llu bytes, out_cap %zu", (unsigned long long)total,
                out_cap);

  // -- C: keys, values and verdicts into the packed output.
  Scratch packed((size_t)total + 16, s);
  if (packed.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%llu bytes of device memory for the results: %s",
                (unsigned long long)total + 16, hipGetErrorString(packed.status()));
  uint8_t* d_out = (uint8_t*)packed.get();
  const bool want_verdict = verdict && internal_keys;
  const GatherArgs ga{e, (const uint64_t*)(e + p_ooff), d_qblock, d_keys, d_koff, d_klen,
                      e + p_called, d_epos, d_rpos, d_fkl, d_vpos, d_vlen, nq, d_out, d_okoff,
                      (uint64_t*)(e + p_voff), (uint64_t*)(e + p_vsrc), (uint32_t*)(e + p_vn),
                      want_verdict ? e + p_verdict : nullptr};
  LGS_HIP(launch_get_gather(ga, s));
  LGS_HIP(launch_pack(e, (const uint64_t*)(e + p_vsrc), (const uint32_t*)(e + p_vn), d_out,
                      (const uint64_t*)(e + p_voff), nq, s));
  if (total) LGS_HIP(hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(out_val_off, e + p_voff, 8 * ((size_t)nq + 1), hipMemcpyDeviceToHost, s));
  if (want_verdict)
    LGS_HIP(hipMemcpyAsync(verdict, e + p_verdict, nq, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  if (verdict && !internal_keys) memset(verdict, kGetNotFound, nq);
  return LGS_OK;
}

// ---- opened tables: ldb_table_open once, ldb_table_internal_get many times
//  ----

// Read-only after lgs_table_open_host: gets from several threads share it.
struct lgs_table {
  int device = -1;
  uint8_t status = LGS_ST_OK;       // why the table did not open, else LGS_ST_OK
  int resident = 0, internal = 0;
  const uint8_t* file = nullptr;    // borrowed when not resident
  uint64_t file_len = 0;
  bool filter = false;              // a filter block that read
  uint32_t index_len = 0;           // the decoded index block
  uint32_t filter_len = 0;          // the filter block as the match takes it
  uint32_t filter_bytes = 0;        // the decoded filter block
  hipStream_t stream = nullptr;     // the stream `mem` was allocated on and is freed on
  std::unique_ptr<Scratch> mem;     // index | filter | lengths | statuses | a zero | image
  uint8_t* d = nullptr;
  size_t d_bytes = 0;
  size_t o_filter = 0, o_olen = 0, o_bst = 0, o_zero = 0, o_img = 0;   // the index block at 0
  // The index entry list, built once by the first scan and
  // read-only from then on: the index block's entries in walk order, on the
  // device (hoff | hsize | state) and on the host, and the walk's end status.
  std::once_flag list_once;
  int list_rc = LGS_OK;
  char list_err[256] = {0};
  std::unique_ptr<Scratch> list_mem;
  uint8_t* list_d = nullptr;
  std::atomic<size_t> list_bytes{0};
  size_t l_hsize = 0, l_state = 0;                 // hoff at 0
  uint32_t list_n = 0;
  uint8_t list_status = LGS_ST_OK;
  std::vector<uint32_t> list_pos;
  std::vector<uint64_t> list_hoff, list_hsize;
  std::vector<uint8_t> list_state;
};

namespace {

// Device scratch of one lgs_table_get / lgs_table_get_dev call before the
// block read, from the library's pool on the call's stream:
//   per query   1 + 1 + 1 + 1 (state, match, seek status, pre)
//               + 8 + 8 (handle) + 5 * 4 (entry, key length, value, restart run)
//               + 4 (qblock) + 8 + 8 + 4 + 4 (a distinct block's handle and room)
//   per byte of the decoded index block   4 (mark) + 8 (rank)
//   8 * scan_parts(max(nq, index_len)) + 8 + 32 (the scans' partial sums, info)
// each array rounded up to 256 bytes; a host call adds its keys + 16 and 12
// bytes a key.  The block read and the results take what lgs_table_get_host's
// second half takes.
struct GetScratch {
  size_t keys = 0, koff = 0, klen = 0, up_end = 0;
  size_t state, match, sst, pre, qhoff, qhsize, epos, fkl, vpos, vlen, rpos, qblock, boff, bsize,
      ocap, room, info, mark, rank, part, total;
  GetScratch(uint32_t nq, uint32_t index_len, bool host, size_t kb) {
    Layout L;
    if (host) {
      keys = L.take(kb + 16);
      koff = L.take(8 * (size_t)nq);
      klen = L.take(4 * (size_t)nq);
    }
    up_end = L.at;
    state = L.take(nq);
    match = L.take(nq);
    sst = L.take(nq);
    pre = L.take(nq);
    qhoff = L.take(8 * (size_t)nq);
    qhsize = L.take(8 * (size_t)nq);
    epos = L.take(4 * (size_t)nq);
    fkl = L.take(4 * (size_t)nq);
    vpos = L.take(4 * (size_t)nq);
    vlen = L.take(4 * (size_t)nq);
    rpos = L.take(lgs_block_seek_scratch(nq));
    qblock = L.take(4 * (size_t)nq);
    boff = L.take(8 * (size_t)nq);
    bsize = L.take(8 * (size_t)nq);
    ocap = L.take(4 * (size_t)nq);
    room = L.take(4 * (size_t)nq);
    info = L.take(32);
    mark = L.take(4 * (size_t)index_len);
    rank = L.take(8 * (size_t)index_len);
    part = L.take(8 * scan_parts(nq > index_len ? nq : index_len) + 8);
    total = L.at;
  }
};

// Where a get's keys come from and where its results go: host memory
// (lgs_table_get) or device memory (lgs_table_get_dev).
struct GetIo {
  bool dev;
  const uint8_t* keys; const uint64_t* key_off; const uint32_t* key_len;
  uint8_t* called; uint8_t* status; uint8_t* verdict; uint8_t* out; size_t out_cap;
  uint64_t* out_key_off; uint64_t* out_val_off; size_t* out_needed;
};

int table_get(lgs_table* t, int verify_checksums, const GetIo& io, uint32_t nq,
              hipStream_t user_stream) {
  if (!t || !io.out_needed || !io.out_key_off || !io.out_val_off)
    return fail(LGS_EINVAL, "NULL argument");
  *io.out_needed = 0;
  if (io.dev && !t->resident)
    return fail(LGS_EINVAL, "lgs_table_get_dev needs a table opened with resident = 1");
  int dev = -1;
  LGS_TRY(call_device(&dev));
  if (dev != t->device)
    return fail(LGS_EINVAL, "table opened on device %d, call on device %d", t->device, dev);
  if (io.dev) {
    LGS_HIP(hipMemsetAsync(io.out_key_off, 0, 8, user_stream));
    LGS_HIP(hipMemsetAsync(io.out_val_off, 0, 8, user_stream));
  } else {
    io.out_key_off[0] = io.out_val_off[0] = 0;
  }
  if (nq == 0) return LGS_OK;
  if (!io.keys || !io.key_off || !io.key_len || !io.called || !io.status ||
      (io.out_cap && !io.out))
    return fail(LGS_EINVAL, "NULL argument");
  if (nq > kMaxEntries) return fail(LGS_EINVAL, "%u queries: under 2^31 supported", nq);
  if (t->status != LGS_ST_OK) {
    if (io.dev) {
      LGS_HIP(launch_get_fail(nq, t->status, io.called, io.status, io.verdict, io.out_key_off,
                              io.out_val_off, user_stream));
      return LGS_OK;
    }
    for (uint32_t q = 0; q < nq; ++q) {
      io.called[q] = 0;
      io.status[q] = t->status;
      if (io.verdict) io.verdict[q] = kGetNotFound;
      io.out_key_off[q + 1] = io.out_val_off[q + 1] = 0;
    }
    return LGS_OK;
  }
  size_t kb = 0;
  if (!io.dev)
    for (uint32_t q = 0; q < nq; ++q) kb += io.key_len[q];
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  hipStream_t s = io.dev ? user_stream : c.stream;
  const uint32_t internal_keys = (uint32_t)t->internal;

  // -- A: the index seek, the handles and the filter on the resident blocks;
  // the live queries' entries marked, ranked and planned on the device.
  const GetScratch G(nq, t->index_len, !io.dev, kb);
  const size_t pin_info = G.up_end, pin_total = G.up_end + 32;
  LGS_TRY(ctx_reserve(c, 0, G.up_end + 64));
  uint8_t* h = c.h_buf;
  Scratch first(G.total, s);
  if (first.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%zu bytes of device memory for %u queries: %s", G.total, nq,
                hipGetErrorString(first.status()));
  uint8_t* d = (uint8_t*)first.get();
  const uint8_t* d_keys = io.keys;
  const uint64_t* d_koff = io.key_off;
  const uint32_t* d_klen = io.key_len;
  if (!io.dev) {
    uint64_t* koff = (uint64_t*)(h + G.koff);
    uint32_t* klen = (uint32_t*)(h + G.klen);
    size_t at = 0;
    for (uint32_t q = 0; q < nq; ++q) {
      koff[q] = at;
      klen[q] = io.key_len[q];
      at += io.key_len[q];
    }
    par_for(nq, kb, [&](uint32_t q0, uint32_t q1) {
      for (uint32_t q = q0; q < q1; ++q)
        memcpy(h + G.keys + koff[q], io.keys + io.key_off[q], io.key_len[q]);
    });
    memset(h + G.keys + kb, 0, 16);
    LGS_HIP(hipMemcpyAsync(d, h, G.up_end, hipMemcpyHostToDevice, s));
    d_keys = d + G.keys;
    d_koff = (const uint64_t*)(d + G.koff);
    d_klen = (const uint32_t*)(d + G.klen);
  }
  uint32_t* d_epos = (uint32_t*)(d + G.epos);
  uint32_t* d_fkl = (uint32_t*)(d + G.fkl);
  uint32_t* d_vpos = (uint32_t*)(d + G.vpos);
  uint32_t* d_vlen = (uint32_t*)(d + G.vlen);
  uint32_t* d_rpos = (uint32_t*)(d + G.rpos);
  uint32_t* d_qblock = (uint32_t*)(d + G.qblock);
  uint64_t* d_boff = (uint64_t*)(d + G.boff);
  uint64_t* d_bsize = (uint64_t*)(d + G.bsize);
  uint32_t* d_ocap = (uint32_t*)(d + G.ocap);
  uint64_t* d_info = (uint64_t*)(d + G.info);
  LGS_HIP(hipMemsetAsync(d + G.info, 0, G.rank - G.info, s));   // info and the marks
  const SeekArgs ia{t->d, (const uint64_t*)(t->d + t->o_zero), (const uint32_t*)(t->d + t->o_olen),
                    t->d + t->o_bst, 1, nullptr, d_keys, d_koff, d_klen, nq, internal_keys,
                    d_epos, d_fkl, d_vpos, d_vlen, d + G.sst, d_rpos, nullptr, nullptr, nullptr};
  LGS_HIP(launch_block_seek(ia, s));
  LGS_HIP(launch_get_handles(t->d, d_epos, d_vpos, d_vlen, nq, (uint64_t*)(d + G.qhoff),
                             (uint64_t*)(d + G.qhsize), d + G.state, s));
  if (t->filter)
    LGS_HIP(launch_filter_block_match(t->d + t->o_filter, t->filter_len,
                                      (const uint64_t*)(d + G.qhoff), d_keys, d_koff, d_klen,
                                      internal_keys ? 8u : 0u, d + G.match, nq, s));
  LGS_HIP(launch_live_mark(d + G.state, t->filter ? d + G.match : nullptr, d + G.sst, d_epos, nq,
                           t->index_len, d + G.pre, d_qblock, (uint32_t*)(d + G.mark), s));
  LGS_HIP(launch_scan(2, nullptr, (const uint32_t*)(d + G.mark), (uint64_t*)(d + G.part), 0,
                      (uint64_t*)(d + G.rank), d_info, t->index_len, s));
  LGS_HIP(launch_qblock((const uint64_t*)(d + G.rank), (const uint64_t*)(d + G.qhoff),
                        (const uint64_t*)(d + G.qhsize), nq, d_qblock, d_boff, d_bsize, s));
  if (t->resident)
    LGS_HIP(launch_block_plan(t->d + t->o_img, t->file_len, d_boff, d_bsize,
                              nq < t->index_len ? nq : t->index_len, d_ocap,
                              (uint32_t*)(d + G.room), d_info, s));
  LGS_HIP(hipMemcpyAsync(h + pin_info, d_info, 32, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));   // the one read-back that sizes the block read
  const uint64_t* info = (const uint64_t*)(h + pin_info);
  if (info[0] > nq)
    return fail(LGS_EINTERNAL, "%llu distinct blocks for %u queries", (unsigned long long)info[0],
                nq);
  const uint32_t nb = (uint32_t)info[0];

  // -- B: the distinct data blocks.
  size_t outb = (size_t)info[1], img = 0;
  uint32_t max_cap = (uint32_t)info[2];
  std::vector<uint64_t> b_off, b_size;
  std::vector<HandlePlan> plan;
  if (t->resident) {
    if (info[3])
      return fail(LGS_EINVAL, "a block of 2^31 bytes or more: under 2^31 supported");
  } else {
    // The distinct handles come down: their byte ranges are staged from the
    // borrowed image, as lgs_table_get_host stages them.
    LGS_TRY(ctx_reserve(c, 0, 16 * (size_t)nb + 64));
    h = c.h_buf;
    if (nb) {
      LGS_HIP(hipMemcpyAsync(h, d_boff, 8 * (size_t)nb, hipMemcpyDeviceToHost, s));
      LGS_HIP(hipMemcpyAsync(h + 8 * (size_t)nb, d_bsize, 8 * (size_t)nb, hipMemcpyDeviceToHost,
                             s));
      LGS_HIP(hipStreamSynchronize(s));
    }
    const uint64_t* ho = (const uint64_t*)h;
    b_off.assign(ho, ho + nb);
    b_size.assign(ho + nb, ho + 2 * (size_t)nb);
    plan.resize(nb);
    for (uint32_t j = 0; j < nb; ++j)
      LGS_TRY(plan_handle(t->file, t->file_len, b_off[j], b_size[j], &plan[j]));
    img = handles_image(b_size.data(), plan.data(), nb, &outb, &max_cap);
  }
  const ReadScratch R(nb);
  Layout B;  // uploads (a borrowed image only) | device-only
  const size_t p_blk = B.take(t->resident ? 0 : img + 32);
  const size_t p_hoff = B.take(8 * (size_t)nb);
  const size_t p_hsize = B.take(8 * (size_t)nb);
  const size_t p_ooff = B.take(8 * (size_t)nb);
  const size_t p_ocap = B.take(4 * (size_t)nb);
  const size_t pin_b = B.at;
  const size_t p_koff = B.take(8 * ((size_t)nq + 1));
  const size_t p_voff = B.take(8 * ((size_t)nq + 1));
  const size_t p_called = B.take(nq);
  const size_t p_fst = B.take(nq);
  const size_t p_verdict = B.take(nq);
  const size_t p_olen = B.take(4 * (size_t)nb);
  const size_t p_bst = B.take(nb);
  const size_t p_len = B.take(4 * (size_t)nq);
  const size_t p_sst = B.take(nq);
  const size_t p_vsrc = B.take(8 * (size_t)nq);
  const size_t p_vn = B.take(4 * (size_t)nq);
  const size_t p_part = B.take(8 * scan_parts(nq > nb ? nq : nb) + 8);
  const size_t p_rscr = B.take(R.total);
  const size_t p_out = B.take(outb + 16);
  Scratch arena(B.at, s);
  if (arena.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%zu bytes of device memory for %u blocks: %s", B.at, nb,
                hipGetErrorString(arena.status()));
  uint8_t* e = (uint8_t*)arena.get();
  if (t->resident) {
    LGS_HIP(launch_scan(2, nullptr, (const uint32_t*)(d + G.room), (uint64_t*)(e + p_part), p_out,
                        (uint64_t*)(e + p_ooff), nullptr, nb, s));
    if (nb)
      LGS_TRY(table_read(t->d + t->o_img, t->file_len, d_boff, d_bsize, nb, verify_checksums, e,
                         (const uint64_t*)(e + p_ooff), d_ocap, max_cap, (uint32_t*)(e + p_olen),
                         e + p_bst, e + p_rscr, R, s));
  } else {
    LGS_TRY(ctx_reserve(c, 0, pin_b + 64));
    h = c.h_buf;
    size_t outb_end = 0;
    stage_handles(t->file, b_off.data(), b_size.data(), plan.data(), nb, h + p_blk,
                  (uint64_t*)(h + p_hoff), (uint64_t*)(h + p_hsize), (uint64_t*)(h + p_ooff),
                  (uint32_t*)(h + p_ocap), p_out, &outb_end);
    LGS_HIP(hipMemcpyAsync(e, h, pin_b, hipMemcpyHostToDevice, s));
    if (nb)
      LGS_TRY(table_read(e + p_blk, img + 16, (const uint64_t*)(e + p_hoff),
                         (const uint64_t*)(e + p_hsize), nb, verify_checksums, e,
                         (const uint64_t*)(e + p_ooff), (const uint32_t*)(e + p_ocap), max_cap,
                         (uint32_t*)(e + p_olen), e + p_bst, e + p_rscr, R, s));
  }
  const SeekArgs da{e, (const uint64_t*)(e + p_ooff), (const uint32_t*)(e + p_olen), e + p_bst, nb,
                    d_qblock, d_keys, d_koff, d_klen, nq, internal_keys, d_epos, d_fkl, d_vpos,
                    d_vlen, e + p_sst, d_rpos, nullptr, nullptr, nullptr};
  LGS_HIP(launch_block_seek(da, s));
  uint8_t* d_called = io.dev ? io.called : e + p_called;
  uint8_t* d_fst = io.dev ? io.status : e + p_fst;
  LGS_HIP(launch_get_lens(d_qblock, d + G.pre, d_epos, d_fkl, d_vlen, e + p_sst, nq, d_called,
                          d_fst, (uint32_t*)(e + p_len), s));
  LGS_HIP(launch_nospace_is_corrupt(d_fst, nq, s));                // plan_handle's cap
  uint64_t* d_okoff = io.dev ? io.out_key_off : (uint64_t*)(e + p_koff);
  uint64_t* d_ovoff = io.dev ? io.out_val_off : (uint64_t*)(e + p_voff);
  LGS_HIP(launch_scan(2, nullptr, (const uint32_t*)(e + p_len), (uint64_t*)(e + p_part), 0, d_okoff,
                      d_okoff + nq, nq, s));
  uint64_t total = 0;
  if (io.dev) {
    h = c.h_buf;
    LGS_HIP(hipMemcpyAsync(h + pin_total, d_okoff + nq, 8, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    total = *(const uint64_t*)(h + pin_total);
  } else {
    LGS_HIP(hipMemcpyAsync(io.out_key_off, d_okoff, 8 * ((size_t)nq + 1), hipMemcpyDeviceToHost,
                           s));
    LGS_HIP(hipMemcpyAsync(io.called, d_called, nq, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipMemcpyAsync(io.status, d_fst, nq, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    total = io.out_key_off[nq];
  }
  *io.out_needed = (size_t)total;
  if (total > io.out_cap)
    return fail(LGS_ENOSPC, "results take %llu bytes, out_cap %zu", (unsigned long long)total,
                io.out_cap);

  // -- C: keys, values and verdicts into the packed output.
  std::unique_ptr<Scratch> packed;
  uint8_t* d_out = io.out;
  if (!io.dev) {
    packed.reset(new Scratch((size_t)total + 16, s));
    if (packed->status() != hipSuccess)
      return fail(LGS_ENOMEM, "%llu bytes of device memory for the results: %s",
                  (unsigned long long)total + 16, hipGetErrorString(packed->status()));
    d_out = (uint8_t*)packed->get();
  }
  const bool want_verdict = io.verdict && internal_keys;
  uint8_t* d_verdict = io.dev ? io.verdict : e + p_verdict;
  const GatherArgs ga{e, (const uint64_t*)(e + p_ooff), d_qblock, d_keys, d_koff, d_klen, d_called,
                      d_epos, d_rpos, d_fkl, d_vpos, d_vlen, nq, d_out, d_okoff, d_ovoff,
                      (uint64_t*)(e + p_vsrc), (uint32_t*)(e + p_vn),
                      want_verdict ? d_verdict : nullptr};
  LGS_HIP(launch_get_gather(ga, s));
  if (total)
    LGS_HIP(launch_pack(e, (const uint64_t*)(e + p_vsrc), (const uint32_t*)(e + p_vn), d_out,
                        d_ovoff, nq, s));
  if (io.dev) {
    // The scratch is freed on the stream behind the work that uses it.
    if (io.verdict && !internal_keys) LGS_HIP(hipMemsetAsync(io.verdict, kGetNotFound, nq, s));
    return LGS_OK;
  }
  if (total) LGS_HIP(hipMemcpyAsync(io.out, d_out, (size_t)total, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(io.out_val_off, d_ovoff, 8 * ((size_t)nq + 1), hipMemcpyDeviceToHost, s));
  if (want_verdict) LGS_HIP(hipMemcpyAsync(io.verdict, d_verdict, nq, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  if (io.verdict && !internal_keys) memset(io.verdict, kGetNotFound, nq);
  return LGS_OK;
}

void table_free(lgs_table* t) {
  if (!t->mem) return;
  int cur = -1;
  const bool moved = hipGetDevice(&cur) == hipSuccess && cur != t->device &&
                     hipSetDevice(t->device) == hipSuccess;
  if (t->list_mem) (void)t->list_mem->release();
  (void)t->mem->release();                 // stream-ordered, then that stream alone is waited on
  (void)hipStreamSynchronize(t->stream);
  t->mem.reset();
  t->list_mem.reset();
  t->d = nullptr;
  t->list_d = nullptr;
  if (moved) (void)hipSetDevice(cur);
}

}  // namespace

int lgs_table_open_host(const uint8_t* file, uint64_t file_len, int paranoid_checks,
                        int internal_keys, const char* filter_name, int resident,
                        lgs_table** table, uint8_t* status) {
  if (!table || !status || !file) return fail(LGS_EINVAL, "NULL argument");
  *table = nullptr;
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  if (resident != 0 && resident != 1) return fail(LGS_EINVAL, "resident must be 0 or 1");
  int dev = -1;
  LGS_TRY(call_device(&dev));
  std::unique_ptr<lgs_table> t(new lgs_table);
  t->device = dev;
  t->resident = resident;
  t->internal = internal_keys;
  t->file = resident ? nullptr : file;
  t->file_len = file_len;
  // ldb_table_open on the host: footer and metaindex.
  uint64_t h2_off[2] = {0, 0}, h2_size[2] = {0, 0};
  uint8_t open_st = LGS_ST_OK;
  LGS_TRY(table_open(file, file_len, paranoid_checks, filter_name, &h2_off[0], &h2_size[0],
                     &h2_off[1], &h2_size[1], &open_st));
  if (open_st != LGS_ST_OK) {
    *status = t->status = open_st;
    *table = t.release();
    return LGS_OK;
  }
  const bool want_filter = h2_off[1] != ~0ull;
  const uint32_t n2 = want_filter ? 2u : 1u;
  HandlePlan plan2[2];
  for (uint32_t j = 0; j < n2; ++j)
    LGS_TRY(plan_handle(file, file_len, h2_off[j], h2_size[j], &plan2[j]));
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  hipStream_t s = c.stream;
  // The index and filter block through table_read, once; what it leaves
  // stays: the decoded blocks, their lengths and statuses.
  size_t out2 = 0;
  uint32_t max_cap2 = 0;
  const size_t img2 = handles_image(h2_size, plan2, n2, &out2, &max_cap2);
  const ReadScratch R2(n2);
  Layout L;  // uploads | device-only
  const size_t o_blk = L.take(img2 + 32);
  const size_t o_hoff = L.take(16);
  const size_t o_hsize = L.take(16);
  const size_t o_ooff = L.take(16);
  const size_t o_ocap = L.take(8);
  const size_t up_end = L.at;
  const size_t o_rscr = L.take(R2.total);
  Layout T;
  T.take(out2 + 16);
  t->o_filter = align_up(plan2[0].cap, 16);
  t->o_olen = T.take(8);
  t->o_bst = T.take(2);
  t->o_zero = T.take(8);
  t->o_img = T.take(resident ? (size_t)file_len + 16 : 0);
  t->d_bytes = T.at;
  LGS_TRY(ctx_reserve(c, 0, up_end + 64));
  uint8_t* h = c.h_buf;
  t->stream = s;
  t->mem.reset(new Scratch(t->d_bytes, s));
  Scratch stage(L.at, s);
  if (t->mem->status() != hipSuccess || stage.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%zu bytes of device memory for the opened table", t->d_bytes + L.at);
  t->d = (uint8_t*)t->mem->get();
  uint8_t* d = (uint8_t*)stage.get();
  size_t out2_end = 0;
  stage_handles(file, h2_off, h2_size, plan2, n2, h + o_blk, (uint64_t*)(h + o_hoff),
                (uint64_t*)(h + o_hsize), (uint64_t*)(h + o_ooff), (uint32_t*)(h + o_ocap), 0,
                &out2_end);
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, s));
  LGS_HIP(hipMemsetAsync(t->d + t->o_olen, 0, t->o_img - t->o_olen, s));
  if (resident) {
    if (file_len) LGS_HIP(hipMemcpyAsync(t->d + t->o_img, file, (size_t)file_len,
                                         hipMemcpyHostToDevice, s));
    LGS_HIP(hipMemsetAsync(t->d + t->o_img + file_len, 0, 16, s));
  }
  LGS_TRY(table_read(d + o_blk, img2 + 16, (const uint64_t*)(d + o_hoff),
                     (const uint64_t*)(d + o_hsize), n2, paranoid_checks, t->d,
                     (const uint64_t*)(d + o_ooff), (const uint32_t*)(d + o_ocap), max_cap2,
                     (uint32_t*)(t->d + t->o_olen), t->d + t->o_bst, d + o_rscr, R2, s));
  LGS_HIP(hipMemcpyAsync(h + up_end, t->d + t->o_olen, 8, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(h + up_end + 8, t->d + t->o_bst, 2, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  const uint32_t* olen = (const uint32_t*)(h + up_end);
  const uint8_t* bst = h + up_end + 8;
  if (bst[0] != LGS_ST_OK) {
    // An index block that does not read: its status for every lookup.
    t->status = bst[0] == LGS_ST_NOSPACE ? (uint8_t)LGS_ST_CORRUPT : bst[0];
    table_free(t.get());
  } else {
    t->index_len = olen[0];
    t->filter = want_filter && bst[1] == LGS_ST_OK;      // table.c:71-72
    t->filter_len = want_filter ? plan2[1].cap : 0;
    t->filter_bytes = t->filter ? olen[1] : 0;
  }
  *status = t->status;
  *table = t.release();
  return LGS_OK;
}

void lgs_table_close(lgs_table* table) {
  if (!table) return;
  table_free(table);
  delete table;
}

int lgs_table_info(const lgs_table* table, uint8_t* status, int* resident, uint64_t* index_bytes,
                   uint64_t* filter_bytes, uint64_t* device_bytes) {
  if (!table) return fail(LGS_EINVAL, "NULL argument");
  if (status) *status = table->status;
  if (resident) *resident = table->resident;
  if (index_bytes) *index_bytes = table->index_len;
  if (filter_bytes) *filter_bytes = table->filter_bytes;
  if (device_bytes) *device_bytes = table->mem ? table->d_bytes + table->list_bytes.load() : 0;
  return LGS_OK;
}

int lgs_table_get(lgs_table* table, int verify_checksums, const uint8_t* keys,
                  const uint64_t* key_off, const uint32_t* key_len, uint32_t nq, uint8_t* called,
                  uint8_t* status, uint8_t* verdict, uint8_t* out, size_t out_cap,
                  uint64_t* out_key_off, uint64_t* out_val_off, size_t* out_needed) {
  const GetIo io{false, keys, key_off, key_len, called, status, verdict, out, out_cap,
                 out_key_off, out_val_off, out_needed};
  return table_get(table, verify_checksums, io, nq, nullptr);
}

int lgs_table_get_dev(lgs_table* table, int verify_checksums, const uint8_t* d_keys,
                      const uint64_t* d_key_off, const uint32_t* d_key_len, uint32_t nq,
                      uint8_t* d_called, uint8_t* d_status, uint8_t* d_verdict, uint8_t* d_out,
                      size_t out_cap, uint64_t* d_out_key_off, uint64_t* d_out_val_off,
                      size_t* out_needed, void* stream) {
  const GetIo io{true, d_keys, d_key_off, d_key_len, d_called, d_status, d_verdict, d_out, out_cap,
                 d_out_key_off, d_out_val_off, out_needed};
  return table_get(table, verify_checksums, io, nq, (hipStream_t)stream);
}

// ---- forward scans: the entries of blocks and of opened tables ----

namespace {

// The scan's device scratch (EntriesScratch, lgs_scan.h) in two parts: what
// the count leaves per block, and what the emit writes per entry (W walked,
// N delivered).
struct EntriesBlockLayout {
  size_t head, wcnt, dcnt, wfirst, dfirst, part, total;
  explicit EntriesBlockLayout(uint32_t nb) {
    Layout L;
    head = L.take(16);
    wcnt = L.take(4 * (size_t)nb);
    dcnt = L.take(4 * (size_t)nb);
    wfirst = L.take(8 * ((size_t)nb + 1));
    dfirst = L.take(8 * ((size_t)nb + 1));
    part = L.take(8 * scan_parts(nb) + 8);
    total = L.at;
  }
};
struct EntriesEntryLayout {
  size_t src, shared, link, eblk, emeta, part, total;
  EntriesEntryLayout(uint64_t W, uint64_t N) {
    Layout L;
    src = L.take(4 * (size_t)W);
    shared = L.take(4 * (size_t)W);
    link = L.take(4 * (size_t)W);
    eblk = L.take(4 * (size_t)N);
    emeta = L.take(4 * (size_t)N);
    part = L.take(8 * scan_parts((uint32_t)N) + 8);
    total = L.at;
  }
};

EntriesScratch entries_scratch(uint8_t* pb, const EntriesBlockLayout& B, uint8_t* pe,
                               const EntriesEntryLayout* E) {
  EntriesScratch w{(uint64_t*)(pb + B.head), (uint32_t*)(pb + B.wcnt), (uint32_t*)(pb + B.dcnt),
                   (uint64_t*)(pb + B.wfirst), (uint64_t*)(pb + B.dfirst), (uint64_t*)(pb + B.part),
                   nullptr, nullptr, nullptr, nullptr, nullptr};
  if (E) {
    w.part = (uint64_t*)(pe + E->part);
    w.src = (uint32_t*)(pe + E->src);
    w.shared = (uint32_t*)(pe + E->shared);
    w.link = (uint32_t*)(pe + E->link);
    w.eblk = (uint32_t*)(pe + E->eblk);
    w.emeta = (uint32_t*)(pe + E->emeta);
  }
  return w;
}

// A block holds at most a third of its bytes in entries.
int entries_bound(uint64_t block_bytes, uint64_t* cap) {
  *cap = block_bytes / 3 + 1;
  if (*cap > kMaxEntries)
    return fail(LGS_EINVAL, "%llu block bytes: under 3 * 2^31 supported",
                (unsigned long long)block_bytes);
  return LGS_OK;
}

}  // namespace

size_t lgs_block_entries_scratch(uint32_t nblocks, uint64_t block_bytes) {
  uint64_t cap = 0;
  if (entries_bound(block_bytes, &cap) != LGS_OK) return 0;
  return EntriesBlockLayout(nblocks).total + EntriesEntryLayout(cap, cap).total;
}

int lgs_block_entries_count_dev(const uint8_t* d_blocks, const uint64_t* d_block_off,
                                const uint32_t* d_block_len, const uint8_t* d_block_status,
                                uint32_t nblocks, uint64_t block_bytes, const uint32_t* d_walk_from,
                                const uint32_t* d_emit_from, int internal_keys,
                                uint32_t* d_entry_first, uint8_t* d_status, uint64_t* d_counts,
                                void* d_scratch, size_t scratch_bytes, void* stream) {
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  if (nblocks > kMaxEntries) return fail(LGS_EINVAL, "%u blocks: under 2^31 supported", nblocks);
  if (!d_entry_first || !d_counts || !d_scratch ||
      (nblocks && (!d_blocks || !d_block_off || !d_block_len || !d_status)))
    return fail(LGS_EINVAL, "NULL argument");
  uint64_t cap = 0;
  LGS_TRY(entries_bound(block_bytes, &cap));
  const EntriesBlockLayout B(nblocks);
  if (scratch_bytes < B.total + EntriesEntryLayout(cap, cap).total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_block_entries_scratch)", scratch_bytes,
                B.total + EntriesEntryLayout(cap, cap).total);
  const EntriesIn in{d_blocks, d_block_off, d_block_len, d_block_status, nblocks, d_walk_from,
                     d_emit_from, (uint32_t)internal_keys};
  LGS_HIP(launch_entries_count(in, entries_scratch((uint8_t*)d_scratch, B, nullptr, nullptr),
                               d_entry_first, d_status, d_counts, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_block_entries_emit_dev(const uint8_t* d_blocks, const uint64_t* d_block_off,
                               const uint32_t* d_block_len, const uint8_t* d_block_status,
                               uint32_t nblocks, uint64_t block_bytes, const uint32_t* d_walk_from,
                               const uint32_t* d_emit_from, int internal_keys, uint32_t n,
                               uint8_t* d_keys, uint64_t* d_key_off, uint32_t* d_key_len,
                               uint8_t* d_vals, uint64_t* d_val_off, uint32_t* d_val_len,
                               void* d_scratch, size_t scratch_bytes, void* stream) {
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  if (nblocks > kMaxEntries) return fail(LGS_EINVAL, "%u blocks: under 2^31 supported", nblocks);
  if (!d_key_off || !d_val_off || !d_scratch ||
      (n && (!d_blocks || !d_block_off || !d_block_len || !d_keys || !d_key_len || !d_vals ||
             !d_val_len)))
    return fail(LGS_EINVAL, "NULL argument");
  uint64_t cap = 0;
  LGS_TRY(entries_bound(block_bytes, &cap));
  if (n > cap) return fail(LGS_EINVAL, "%u entries in %llu block bytes", n,
                           (unsigned long long)block_bytes);
  const EntriesBlockLayout B(nblocks);
  const EntriesEntryLayout E(cap, cap);
  if (scratch_bytes < B.total + E.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_block_entries_scratch)", scratch_bytes,
                B.total + E.total);
  const EntriesIn in{d_blocks, d_block_off, d_block_len, d_block_status, nblocks, d_walk_from,
                     d_emit_from, (uint32_t)internal_keys};
  uint8_t* p = (uint8_t*)d_scratch;
  LGS_HIP(launch_entries_emit(in, entries_scratch(p, B, p + B.total, &E), cap, n, d_keys, d_key_off,
                              d_key_len, d_vals, d_val_off, d_val_len, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_block_entries_host(const uint8_t* blocks, const uint64_t* block_off,
                           const uint32_t* block_len, const uint8_t* block_status, uint32_t nblocks,
                           const uint32_t* walk_from, const uint32_t* emit_from, int internal_keys,
                           uint32_t* entry_first, uint8_t* status, uint8_t* keys, size_t key_cap,
                           uint64_t* key_off, uint32_t* key_len, uint8_t* vals, size_t val_cap,
                           uint64_t* val_off, uint32_t* val_len, uint32_t entry_cap,
                           uint64_t* needed) {
  if (internal_keys != 0 && internal_keys != 1)
    return fail(LGS_EINVAL, "internal_keys must be 0 or 1");
  if (nblocks > kMaxEntries) return fail(LGS_EINVAL, "%u blocks: under 2^31 supported", nblocks);
  if (!entry_first || !key_off || !val_off || !needed ||
      (nblocks && (!blocks || !block_off || !block_len || !status)))
    return fail(LGS_EINVAL, "NULL argument");
  needed[0] = needed[1] = needed[2] = 0;
  entry_first[0] = 0;
  key_off[0] = val_off[0] = 0;
  if (nblocks == 0) return LGS_OK;
  size_t bb = 0;
  for (uint32_t b = 0; b < nblocks; ++b) bb += block_len[b];
  uint64_t cap = 0;
  LGS_TRY(entries_bound(bb, &cap));
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  hipStream_t s = c.stream;
  const EntriesBlockLayout B(nblocks);
  Layout L;  // uploads | downloads | device-only
  const size_t o_blk = L.take(bb + 16);
  const size_t o_boff = L.take(8 * (size_t)nblocks);
  const size_t o_blen = L.take(4 * (size_t)nblocks);
  const size_t o_bst = L.take(nblocks);
  const size_t o_wf = L.take(4 * (size_t)nblocks);
  const size_t o_ef = L.take(4 * (size_t)nblocks);
  const size_t up_end = L.at;
  const size_t o_cnt = L.take(8 * kEntryCounts);      // downloads
  const size_t o_head = L.take(16);
  const size_t o_first = L.take(4 * ((size_t)nblocks + 1));
  const size_t o_st = L.take(nblocks);
  const size_t pin_end = L.at;
  const size_t o_scr = L.take(B.total);
  LGS_TRY(ctx_reserve(c, L.at, pin_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  {
    uint64_t* boff = (uint64_t*)(h + o_boff);
    size_t at = 0;
    for (uint32_t b = 0; b < nblocks; ++b) {
      boff[b] = at;
      at += block_len[b];
    }
    memcpy(h + o_blen, block_len, 4 * (size_t)nblocks);
    par_for(nblocks, bb, [&](uint32_t b0, uint32_t b1) {
      for (uint32_t b = b0; b < b1; ++b) memcpy(h + o_blk + boff[b], blocks + block_off[b], block_len[b]);
    });
    memset(h + o_blk + bb, 0, 16);
    if (block_status) memcpy(h + o_bst, block_status, nblocks);
    if (walk_from) memcpy(h + o_wf, walk_from, 4 * (size_t)nblocks);
    if (emit_from) memcpy(h + o_ef, emit_from, 4 * (size_t)nblocks);
  }
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, s));
  const EntriesIn in{d + o_blk, (const uint64_t*)(d + o_boff), (const uint32_t*)(d + o_blen),
                     block_status ? d + o_bst : nullptr, nblocks,
                     walk_from ? (const uint32_t*)(d + o_wf) : nullptr,
                     emit_from ? (const uint32_t*)(d + o_ef) : nullptr, (uint32_t)internal_keys};
  const EntriesScratch w0 = entries_scratch(d + o_scr, B, nullptr, nullptr);
  uint64_t* d_cnt = (uint64_t*)(d + o_cnt);
  LGS_HIP(launch_entries_count(in, w0, (uint32_t*)(d + o_first), d + o_st, d_cnt, s));
  LGS_HIP(hipMemcpyAsync(d + o_head, w0.head, 16, hipMemcpyDeviceToDevice, s));
  LGS_HIP(hipMemcpyAsync(h + o_cnt, d + o_cnt, pin_end - o_cnt, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));   // the one read-back that sizes the outputs
  const uint64_t* cnt = (const uint64_t*)(h + o_cnt);
  const uint64_t walked = *(const uint64_t*)(h + o_head);
  const uint64_t n = cnt[0], kb = cnt[1], vb = cnt[2];
  memcpy(entry_first, h + o_first, 4 * ((size_t)nblocks + 1));
  memcpy(status, h + o_st, nblocks);
  needed[0] = n;
  needed[1] = kb;
  needed[2] = vb;
  if (walked > cap || n > walked)
    return fail(LGS_EINTERNAL, "%llu entries walked, %llu delivered in %zu block bytes",
                (unsigned long long)walked, (unsigned long long)n, bb);
  if (n > entry_cap || kb > key_cap || vb > val_cap)
    return fail(LGS_ENOSPC, "%llu entries (entry_cap %u), keys %llu bytes (key_cap %zu), values %llu (val_cap %zu)",
                (unsigned long long)n, entry_cap, (unsigned long long)kb, key_cap,
                (unsigned long long)vb, val_cap);
  if (n == 0) return LGS_OK;
  const EntriesEntryLayout E(walked, n);
  Layout O;  // downloads | device-only
  const size_t q_keys = O.take((size_t)kb + 16);
  const size_t q_vals = O.take((size_t)vb + 16);
  const size_t q_koff = O.take(8 * ((size_t)n + 1));
  const size_t q_voff = O.take(8 * ((size_t)n + 1));
  const size_t q_klen = O.take(4 * (size_t)n);
  const size_t q_vlen = O.take(4 * (size_t)n);
  const size_t q_end = O.at;
  const size_t q_scr = O.take(E.total);
  Scratch arena(O.at, s);
  if (arena.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%zu bytes of device memory for %llu entries: %s", O.at,
                (unsigned long long)n, hipGetErrorString(arena.status()));
  uint8_t* e = (uint8_t*)arena.get();
  LGS_HIP(launch_entries_emit(in, entries_scratch(d + o_scr, B, e + q_scr, &E), walked, (uint32_t)n,
                              e + q_keys, (uint64_t*)(e + q_koff), (uint32_t*)(e + q_klen),
                              e + q_vals, (uint64_t*)(e + q_voff), (uint32_t*)(e + q_vlen), s));
  LGS_TRY(ctx_reserve(c, 0, q_end));
  h = c.h_buf;
  LGS_HIP(hipMemcpyAsync(h, e, q_end, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  memcpy(keys, h + q_keys, (size_t)kb);
  memcpy(vals, h + q_vals, (size_t)vb);
  memcpy(key_off, h + q_koff, 8 * ((size_t)n + 1));
  memcpy(val_off, h + q_voff, 8 * ((size_t)n + 1));
  memcpy(key_len, h + q_klen, 4 * (size_t)n);
  memcpy(val_len, h + q_vlen, 4 * (size_t)n);
  return LGS_OK;
}

namespace {

// The index entry arrays of launch_index_slots / launch_index_walk inside one
// allocation of `cap` entries.
struct IndexListLayout {
  size_t hoff, hsize, state, pos, info, total;
  explicit IndexListLayout(size_t cap) {
    Layout L;
    hoff = L.take(8 * cap);
    hsize = L.take(8 * cap);
    state = L.take(cap);
    pos = L.take(4 * cap);
    info = L.take(32);
    total = L.at;
  }
  IndexList at(uint8_t* p) const {
    return IndexList{(uint32_t*)(p + pos), (uint64_t*)(p + hoff), (uint64_t*)(p + hsize), p + state,
                     (uint64_t*)(p + info)};
  }
};

// Builds the handle's index entry list on stream s (std::call_once's body).
int index_list_build(lgs_table* t, Ctx& c, hipStream_t s) {
  const size_t cap = (size_t)t->index_len / 3 + 1;
  const IndexListLayout T(cap);
  LGS_TRY(ctx_reserve(c, 0, T.total + 64));
  uint8_t* h = c.h_buf;
  Scratch tmp(T.total, s);
  if (tmp.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%zu bytes of device memory for the index entries", T.total);
  uint8_t* d = (uint8_t*)tmp.get();
  const IndexList out = T.at(d);
  const uint64_t* info = (const uint64_t*)(h + T.info);
  LGS_HIP(launch_index_slots(t->d, t->index_len, (uint32_t)t->internal, (uint32_t)cap, out, s));
  LGS_HIP(hipMemcpyAsync(h + T.info, d + T.info, 32, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  if (info[2]) {
    // The slots disagree: the single-lane walk, exact for any contents.
    LGS_HIP(launch_index_walk(t->d, t->index_len, (uint32_t)t->internal, kNoOffset, (uint32_t)cap,
                              out, s));
    LGS_HIP(hipMemcpyAsync(h + T.info, d + T.info, 32, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
  }
  if (info[0] > cap) return fail(LGS_EINTERNAL, "%llu index entries in %u bytes",
                                 (unsigned long long)info[0], t->index_len);
  const uint32_t n = (uint32_t)info[0];
  const uint8_t st = (uint8_t)info[1];
  Layout F;
  F.take(8 * (size_t)n);
  const size_t l_hsize = F.take(8 * (size_t)n);
  const size_t l_state = F.take((size_t)n + 16);
  // From the handle's pool, on its stream; that stream alone is waited on
  // before the copy on s.
  t->list_mem.reset(new Scratch(F.at, t->stream));
  if (t->list_mem->status() != hipSuccess) {
    t->list_mem.reset();
    return fail(LGS_ENOMEM, "%zu bytes of device memory for the index entries", F.at);
  }
  LGS_HIP(hipStreamSynchronize(t->stream));
  uint8_t* ld = (uint8_t*)t->list_mem->get();
  if (n) {
    LGS_HIP(hipMemcpyAsync(ld, d + T.hoff, 8 * (size_t)n, hipMemcpyDeviceToDevice, s));
    LGS_HIP(hipMemcpyAsync(ld + l_hsize, d + T.hsize, 8 * (size_t)n, hipMemcpyDeviceToDevice, s));
    LGS_HIP(hipMemcpyAsync(ld + l_state, d + T.state, n, hipMemcpyDeviceToDevice, s));
    LGS_HIP(hipMemcpyAsync(h + T.hoff, d + T.hoff, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipMemcpyAsync(h + T.hsize, d + T.hsize, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipMemcpyAsync(h + T.state, d + T.state, n, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipMemcpyAsync(h + T.pos, d + T.pos, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    const uint64_t* ho = (const uint64_t*)(h + T.hoff);
    const uint64_t* hs = (const uint64_t*)(h + T.hsize);
    const uint32_t* po = (const uint32_t*)(h + T.pos);
    t->list_hoff.assign(ho, ho + n);
    t->list_hsize.assign(hs, hs + n);
    t->list_state.assign(h + T.state, h + T.state + n);
    t->list_pos.assign(po, po + n);
  }
  t->list_d = ld;
  t->l_hsize = l_hsize;
  t->l_state = l_state;
  t->list_n = n;
  t->list_status = st;
  t->list_bytes.store(F.at);
  return LGS_OK;
}

int index_list(lgs_table* t, Ctx& c, hipStream_t s) {
  std::call_once(t->list_once, [&] {
    t->list_rc = index_list_build(t, c, s);
    if (t->list_rc != LGS_OK) snprintf(t->list_err, sizeof t->list_err, "%s", t_err);
  });
  if (t->list_rc != LGS_OK) return fail(t->list_rc, "%s", t->list_err);
  return LGS_OK;
}

// Where a scan's start comes from and where its results go: host memory
// (lgs_table_scan) or device memory (lgs_table_scan_dev; the start key and
// the scalar results stay host words).
struct ScanIo {
  bool dev;
  const uint8_t* start; uint32_t start_len; int has_start;
  uint32_t first_block, max_blocks;
  uint8_t* keys; size_t key_cap; uint64_t* key_off; uint32_t* key_len;
  uint8_t* vals; size_t val_cap; uint64_t* val_off; uint32_t* val_len; uint32_t entry_cap;
  uint32_t* block_entry_first; uint8_t* block_status;
  uint32_t* blocks_done; uint32_t* next_block; int* at_end; uint8_t* index_status;
  uint64_t* needed;
};

int table_scan(lgs_table* t, int verify_checksums, const ScanIo& io, hipStream_t user_stream) {
  if (!t || !io.blocks_done || !io.next_block || !io.at_end || !io.index_status || !io.needed ||
      !io.key_off || !io.val_off || !io.block_entry_first)
    return fail(LGS_EINVAL, "NULL argument");
  if (io.has_start && !io.start && io.start_len) return fail(LGS_EINVAL, "NULL argument");
  if (io.max_blocks == 0 || io.max_blocks > kMaxEntries)
    return fail(LGS_EINVAL, "max_blocks must be at least 1 and under 2^31");
  if (io.dev && !t->resident)
    return fail(LGS_EINVAL, "lgs_table_scan_dev needs a table opened with resident = 1");
  int dev = -1;
  LGS_TRY(call_device(&dev));
  if (dev != t->device)
    return fail(LGS_EINVAL, "table opened on device %d, call on device %d", t->device, dev);
  *io.blocks_done = 0;
  *io.next_block = io.first_block;
  *io.at_end = 1;
  *io.index_status = t->status;
  io.needed[0] = io.needed[1] = io.needed[2] = io.needed[3] = 0;
  const size_t slack = io.dev ? 16 : 0;
  auto no_entries = [&]() -> int {
    if (io.dev) {
      LGS_HIP(hipMemsetAsync(io.key_off, 0, 8, user_stream));
      LGS_HIP(hipMemsetAsync(io.val_off, 0, 8, user_stream));
      LGS_HIP(hipMemsetAsync(io.block_entry_first, 0, 4, user_stream));
    } else {
      io.key_off[0] = io.val_off[0] = 0;
      io.block_entry_first[0] = 0;
    }
    return LGS_OK;
  };
  if (t->status != LGS_ST_OK) return no_entries();   // a table that did not open: no iterator
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  hipStream_t s = io.dev ? user_stream : c.stream;
  const uint32_t internal_keys = (uint32_t)t->internal;
  LGS_TRY(index_list(t, c, s));
  *io.index_status = t->list_status;

  // -- A: the window of index entries.  With a start key, ldb_twoiter_seek's
  // index seek names its first entry.
  const uint64_t* w_hoff = t->list_hoff.data();       // the window's entries on the host ...
  const uint64_t* w_hsize = t->list_hsize.data();
  const uint8_t* w_state = t->list_state.data();
  const uint8_t* dl = t->list_d;                      // ... and on the device
  const uint64_t* dw_hoff = (const uint64_t*)dl;
  const uint64_t* dw_hsize = (const uint64_t*)(dl + t->l_hsize);
  const uint8_t* dw_state = dl + t->l_state;
  uint32_t b0 = io.first_block, nb = 0, next = 0;
  bool at_end = true;
  std::unique_ptr<Scratch> seek_mem, side_mem;
  std::vector<uint64_t> side_hoff, side_hsize;
  std::vector<uint8_t> side_state;
  const uint8_t* d_start = nullptr;                   // the start key on the device
  const uint64_t* d_start_off = nullptr;
  const uint32_t* d_start_len = nullptr;
  uint8_t* sk = nullptr;                              // the seeks' outputs
  Layout S;
  const size_t s_key = S.take((size_t)io.start_len + 16);
  const size_t s_koff = S.take(8);
  const size_t s_klen = S.take(4);
  const size_t s_up = S.at;
  const size_t s_epos = S.take(4);
  const size_t s_sst = S.take(4);
  const size_t s_down = S.at;
  const size_t s_fkl = S.take(4);
  const size_t s_vpos = S.take(4);
  const size_t s_vlen = S.take(4);
  const size_t s_rpos = S.take(lgs_block_seek_scratch(1));
  if (io.has_start) {
    LGS_TRY(ctx_reserve(c, 0, s_down + 64));
    uint8_t* h = c.h_buf;
    seek_mem.reset(new Scratch(S.at, s));
    if (seek_mem->status() != hipSuccess)
      return fail(LGS_ENOMEM, "%zu bytes of device memory for the seek", S.at);
    sk = (uint8_t*)seek_mem->get();
    memset(h, 0, s_up);
    if (io.start_len) memcpy(h + s_key, io.start, io.start_len);
    *(uint32_t*)(h + s_klen) = io.start_len;
    LGS_HIP(hipMemcpyAsync(sk, h, s_up, hipMemcpyHostToDevice, s));
    d_start = sk + s_key;
    d_start_off = (const uint64_t*)(sk + s_koff);
    d_start_len = (const uint32_t*)(sk + s_klen);
    const SeekArgs ia{t->d, (const uint64_t*)(t->d + t->o_zero), (const uint32_t*)(t->d + t->o_olen),
                      t->d + t->o_bst, 1, nullptr, d_start, d_start_off, d_start_len, 1,
                      internal_keys, (uint32_t*)(sk + s_epos), (uint32_t*)(sk + s_fkl),
                      (uint32_t*)(sk + s_vpos), (uint32_t*)(sk + s_vlen), sk + s_sst,
                      (uint32_t*)(sk + s_rpos), nullptr, nullptr, nullptr};
    LGS_HIP(launch_block_seek(ia, s));
    LGS_HIP(hipMemcpyAsync(h + s_epos, sk + s_epos, s_down - s_epos, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    const uint32_t epos = *(const uint32_t*)(h + s_epos);
    if (epos == kNoEntry) {
      // An invalid index iterator: no block, and its status is the scan's.
      *io.index_status = h[s_sst];
      *io.next_block = t->list_n;
      return no_entries();
    }
    const auto it = std::lower_bound(t->list_pos.begin(), t->list_pos.end(), epos);
    if (it != t->list_pos.end() && *it == epos) {
      b0 = (uint32_t)(it - t->list_pos.begin());
    } else {
      // The seek's entry is none the walk from restart[0] visits (a damaged
      // index block): the entries from it up to where the two walks meet, by
      // the serial walk, in one window.
      const size_t cap = (size_t)t->index_len / 3 + 1;
      const IndexListLayout T(cap);
      LGS_TRY(ctx_reserve(c, 0, T.total + 64));
      h = c.h_buf;
      side_mem.reset(new Scratch(T.total, s));
      if (side_mem->status() != hipSuccess)
        return fail(LGS_ENOMEM, "%zu bytes of device memory for the index entries", T.total);
      uint8_t* sd = (uint8_t*)side_mem->get();
      LGS_HIP(launch_index_walk(t->d, t->index_len, internal_keys, epos, (uint32_t)cap, T.at(sd), s));
      LGS_HIP(hipMemcpyAsync(h, sd, T.total, hipMemcpyDeviceToHost, s));
      LGS_HIP(hipStreamSynchronize(s));
      const uint64_t* info = (const uint64_t*)(h + T.info);
      const uint32_t* po = (const uint32_t*)(h + T.pos);
      uint32_t k = 0, join = t->list_n;
      bool joined = false;
      for (; k < info[0]; ++k) {
        const auto j = std::lower_bound(t->list_pos.begin(), t->list_pos.end(), po[k]);
        if (j != t->list_pos.end() && *j == po[k]) {
          join = (uint32_t)(j - t->list_pos.begin());
          joined = true;
          break;
        }
      }
      if (k > io.max_blocks) {
        io.needed[3] = k;
        return fail(LGS_ENOSPC, "the seek's window takes %u blocks, max_blocks %u", k, io.max_blocks);
      }
      const uint64_t* ho = (const uint64_t*)(h + T.hoff);
      const uint64_t* hs = (const uint64_t*)(h + T.hsize);
      side_hoff.assign(ho, ho + k);
      side_hsize.assign(hs, hs + k);
      side_state.assign(h + T.state, h + T.state + k);
      w_hoff = side_hoff.data();
      w_hsize = side_hsize.data();
      w_state = side_state.data();
      dw_hoff = (const uint64_t*)(sd + T.hoff);
      dw_hsize = (const uint64_t*)(sd + T.hsize);
      dw_state = sd + T.state;
      b0 = 0;
      nb = k;
      next = join;
      at_end = !joined;
      if (!joined) *io.index_status = (uint8_t)info[1];
    }
  }
  if (!side_mem) {
    if (b0 > t->list_n) b0 = t->list_n;
    nb = t->list_n - b0 < io.max_blocks ? t->list_n - b0 : io.max_blocks;
    next = b0 + nb;
    at_end = next >= t->list_n;
    w_hoff += b0;
    w_hsize += b0;
    w_state += b0;
    dw_hoff += b0;
    dw_hsize += b0;
    dw_state += b0;
  }
  *io.blocks_done = nb;
  *io.next_block = next;
  *io.at_end = at_end ? 1 : 0;
  if (nb == 0) return no_entries();

  // -- B: the window's blocks, read as a get reads its distinct blocks.
  const EntriesBlockLayout EB(nb);
  Layout P;  // resident: the plan, device-only
  const size_t p_ocap = P.take(4 * (size_t)nb);
  const size_t p_room = P.take(4 * (size_t)nb);
  const size_t p_info = P.take(32);
  size_t outb = 0, img = 0;
  uint32_t max_cap = 0;
  std::unique_ptr<Scratch> plan_mem;
  std::vector<HandlePlan> plan;
  uint8_t* pd = nullptr;
  if (t->resident) {
    LGS_TRY(ctx_reserve(c, 0, 64));
    uint8_t* h = c.h_buf;
    plan_mem.reset(new Scratch(P.at, s));
    if (plan_mem->status() != hipSuccess)
      return fail(LGS_ENOMEM, "%zu bytes of device memory for %u blocks", P.at, nb);
    pd = (uint8_t*)plan_mem->get();
    LGS_HIP(launch_plan_info((uint64_t*)(pd + p_info), nb, s));
    LGS_HIP(launch_block_plan(t->d + t->o_img, t->file_len, dw_hoff, dw_hsize, nb,
                              (uint32_t*)(pd + p_ocap), (uint32_t*)(pd + p_room),
                              (uint64_t*)(pd + p_info), s));
    LGS_HIP(hipMemcpyAsync(h, pd + p_info, 32, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));   // the read-back that sizes the block read
    const uint64_t* info = (const uint64_t*)h;
    if (info[3]) return fail(LGS_EINVAL, "a block of 2^31 bytes or more: under 2^31 supported");
    outb = (size_t)info[1];
    max_cap = (uint32_t)info[2];
  } else {
    plan.resize(nb);
    for (uint32_t j = 0; j < nb; ++j)
      LGS_TRY(plan_handle(t->file, t->file_len, w_hoff[j], w_hsize[j], &plan[j]));
    img = handles_image(w_hsize, plan.data(), nb, &outb, &max_cap);
  }
  const ReadScratch R(nb);
  Layout B;  // uploads (a borrowed image only) | downloads | device-only
  const size_t p_blk = B.take(t->resident ? 0 : img + 32);
  const size_t p_hoff = B.take(8 * (size_t)nb);
  const size_t p_hsize = B.take(8 * (size_t)nb);
  const size_t p_ooff = B.take(8 * (size_t)nb);
  const size_t p_ocap2 = B.take(4 * (size_t)nb);
  const size_t p_state = B.take(nb);
  const size_t pin_b = B.at;
  const size_t p_cnt = B.take(8 * kEntryCounts);      // downloads
  const size_t p_head = B.take(16);
  const size_t p_first = B.take(4 * ((size_t)nb + 1));
  const size_t p_st = B.take(nb);
  const size_t down_end = B.at;
  const size_t p_olen = B.take(4 * (size_t)nb);
  const size_t p_bst = B.take(nb);
  const size_t p_wf = B.take(4 * (size_t)nb);
  const size_t p_ef = B.take(4 * (size_t)nb);
  const size_t p_part = B.take(8 * scan_parts(nb) + 8);
  const size_t p_rscr = B.take(R.total);
  const size_t p_escr = B.take(EB.total);
  const size_t p_out = B.take(outb + 16);
  LGS_TRY(ctx_reserve(c, 0, std::max(pin_b, down_end - p_cnt) + 64));
  uint8_t* h = c.h_buf;
  Scratch arena(B.at, s);
  if (arena.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%zu bytes of device memory for %u blocks: %s", B.at, nb,
                hipGetErrorString(arena.status()));
  uint8_t* e = (uint8_t*)arena.get();
  const uint8_t* d_state = dw_state;
  if (t->resident) {
    LGS_HIP(launch_scan(2, nullptr, (const uint32_t*)(pd + p_room), (uint64_t*)(e + p_part), p_out,
                        (uint64_t*)(e + p_ooff), nullptr, nb, s));
    LGS_TRY(table_read(t->d + t->o_img, t->file_len, dw_hoff, dw_hsize, nb, verify_checksums, e,
                       (const uint64_t*)(e + p_ooff), (const uint32_t*)(pd + p_ocap), max_cap,
                       (uint32_t*)(e + p_olen), e + p_bst, e + p_rscr, R, s));
  } else {
    size_t outb_end = 0;
    stage_handles(t->file, w_hoff, w_hsize, plan.data(), nb, h + p_blk, (uint64_t*)(h + p_hoff),
                  (uint64_t*)(h + p_hsize), (uint64_t*)(h + p_ooff), (uint32_t*)(h + p_ocap2), p_out,
                  &outb_end);
    memcpy(h + p_state, w_state, nb);
    LGS_HIP(hipMemcpyAsync(e, h, pin_b, hipMemcpyHostToDevice, s));
    LGS_TRY(table_read(e + p_blk, img + 16, (const uint64_t*)(e + p_hoff),
                       (const uint64_t*)(e + p_hsize), nb, verify_checksums, e,
                       (const uint64_t*)(e + p_ooff), (const uint32_t*)(e + p_ocap2), max_cap,
                       (uint32_t*)(e + p_olen), e + p_bst, e + p_rscr, R, s));
    d_state = e + p_state;
  }
  LGS_HIP(launch_scan_status(d_state, e + p_bst, nb, s));
  const uint32_t* d_wf = nullptr;
  const uint32_t* d_ef = nullptr;
  if (io.has_start) {
    // ldb_twoiter_seek's data seek: a fresh iterator on the window's first
    // block; the scan goes on from the entry it found, in the restart run it
    // chose.
    LGS_HIP(hipMemsetAsync(e + p_wf, 0xff, p_part - p_wf, s));
    const SeekArgs da{e, (const uint64_t*)(e + p_ooff), (const uint32_t*)(e + p_olen), e + p_bst, nb,
                      nullptr, d_start, d_start_off, d_start_len, 1, internal_keys,
                      (uint32_t*)(sk + s_epos), (uint32_t*)(sk + s_fkl), (uint32_t*)(sk + s_vpos),
                      (uint32_t*)(sk + s_vlen), sk + s_sst, (uint32_t*)(sk + s_rpos), nullptr,
                      nullptr, nullptr};
    LGS_HIP(launch_block_seek(da, s));
    LGS_HIP(launch_scan_seek_apply((const uint32_t*)(sk + s_epos), (const uint32_t*)(sk + s_rpos),
                                   sk + s_sst, (uint32_t*)(e + p_wf), (uint32_t*)(e + p_ef),
                                   e + p_bst, s));
    d_wf = (const uint32_t*)(e + p_wf);
    d_ef = (const uint32_t*)(e + p_ef);
  }

  // -- C: the entries (§2's two calls around the read-back of the counts).
  const EntriesIn in{e, (const uint64_t*)(e + p_ooff), (const uint32_t*)(e + p_olen), e + p_bst, nb,
                     d_wf, d_ef, internal_keys};
  const EntriesScratch w0 = entries_scratch(e + p_escr, EB, nullptr, nullptr);
  uint32_t* d_first = io.dev ? io.block_entry_first : (uint32_t*)(e + p_first);
  uint8_t* d_st = io.dev ? io.block_status : e + p_st;
  LGS_HIP(launch_entries_count(in, w0, d_first, d_st, (uint64_t*)(e + p_cnt), s));
  LGS_HIP(hipMemcpyAsync(e + p_head, w0.head, 16, hipMemcpyDeviceToDevice, s));
  LGS_HIP(hipMemcpyAsync(h, e + p_cnt, (io.dev ? p_first : down_end) - p_cnt, hipMemcpyDeviceToHost,
                         s));
  LGS_HIP(hipStreamSynchronize(s));   // the read-back that sizes the outputs
  const uint64_t* cnt = (const uint64_t*)h;
  const uint64_t walked = *(const uint64_t*)(h + (p_head - p_cnt));
  const uint64_t n = cnt[0], kb = cnt[1], vb = cnt[2];
  if (!io.dev) {
    memcpy(io.block_entry_first, h + (p_first - p_cnt), 4 * ((size_t)nb + 1));
    if (io.block_status) memcpy(io.block_status, h + (p_st - p_cnt), nb);
  }
  io.needed[0] = n;
  io.needed[1] = kb + slack;
  io.needed[2] = vb + slack;
  if (walked > kMaxEntries || n > walked)
    return fail(LGS_EINVAL, "%llu entries in one window: under 2^31 supported",
                (unsigned long long)walked);
  if (n > io.entry_cap || kb + slack > io.key_cap || vb + slack > io.val_cap)
    return fail(LGS_ENOSPC, "%llu entries (entry_cap %u), keys %llu bytes (key_cap %zu), values %llu (val_cap %zu)",
                (unsigned long long)n, io.entry_cap, (unsigned long long)(kb + slack), io.key_cap,
                (unsigned long long)(vb + slack), io.val_cap);
  if (n == 0) {
    if (io.dev) {
      LGS_HIP(hipMemsetAsync(io.key_off, 0, 8, s));
      LGS_HIP(hipMemsetAsync(io.val_off, 0, 8, s));
    } else {
      io.key_off[0] = io.val_off[0] = 0;
    }
    return LGS_OK;
  }
  if (!io.keys || !io.key_len || !io.vals || !io.val_len) return fail(LGS_EINVAL, "NULL argument");
  const EntriesEntryLayout EE(walked, n);
  Layout O;  // downloads (a host call only) | device-only
  const size_t q_keys = O.take(io.dev ? 0 : (size_t)kb + 16);
  const size_t q_vals = O.take(io.dev ? 0 : (size_t)vb + 16);
  const size_t q_koff = O.take(io.dev ? 0 : 8 * ((size_t)n + 1));
  const size_t q_voff = O.take(io.dev ? 0 : 8 * ((size_t)n + 1));
  const size_t q_klen = O.take(io.dev ? 0 : 4 * (size_t)n);
  const size_t q_vlen = O.take(io.dev ? 0 : 4 * (size_t)n);
  const size_t q_end = O.at;
  const size_t q_scr = O.take(EE.total);
  Scratch second(O.at, s);
  if (second.status() != hipSuccess)
    return fail(LGS_ENOMEM, "%zu bytes of device memory for %llu entries: %s", O.at,
                (unsigned long long)n, hipGetErrorString(second.status()));
  uint8_t* g = (uint8_t*)second.get();
  const EntriesScratch w1 = entries_scratch(e + p_escr, EB, g + q_scr, &EE);
  if (io.dev) {
    // The scratch is freed on the stream behind the work that uses it.
    LGS_HIP(launch_entries_emit(in, w1, walked, (uint32_t)n, io.keys, io.key_off, io.key_len, io.vals,
                                io.val_off, io.val_len, s));
    return LGS_OK;
  }
  LGS_HIP(launch_entries_emit(in, w1, walked, (uint32_t)n, g + q_keys, (uint64_t*)(g + q_koff),
                              (uint32_t*)(g + q_klen), g + q_vals, (uint64_t*)(g + q_voff),
                              (uint32_t*)(g + q_vlen), s));
  LGS_TRY(ctx_reserve(c, 0, q_end));
  h = c.h_buf;
  LGS_HIP(hipMemcpyAsync(h, g, q_end, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  memcpy(io.keys, h + q_keys, (size_t)kb);
  memcpy(io.vals, h + q_vals, (size_t)vb);
  memcpy(io.key_off, h + q_koff, 8 * ((size_t)n + 1));
  memcpy(io.val_off, h + q_voff, 8 * ((size_t)n + 1));
  memcpy(io.key_len, h + q_klen, 4 * (size_t)n);
  memcpy(io.val_len, h + q_vlen, 4 * (size_t)n);
  return LGS_OK;
}

}  // namespace

int lgs_table_scan(lgs_table* table, int verify_checksums, const uint8_t* start,
                   uint32_t start_len, int has_start, uint32_t first_block, uint32_t max_blocks,
                   uint8_t* keys, size_t key_cap, uint64_t* key_off, uint32_t* key_len,
                   uint8_t* vals, size_t val_cap, uint64_t* val_off, uint32_t* val_len,
                   uint32_t entry_cap, uint32_t* block_entry_first, uint8_t* block_status,
                   uint32_t* blocks_done, uint32_t* next_block, int* at_end, uint8_t* index_status,
                   uint64_t* needed) {
  const ScanIo io{false, start, start_len, has_start, first_block, max_blocks, keys, key_cap,
                  key_off, key_len, vals, val_cap, val_off, val_len, entry_cap, block_entry_first,
                  block_status, blocks_done, next_block, at_end, index_status, needed};
  return table_scan(table, verify_checksums, io, nullptr);
}

int lgs_table_scan_dev(lgs_table* table, int verify_checksums, const uint8_t* start,
                       uint32_t start_len, int has_start, uint32_t first_block,
                       uint32_t max_blocks, uint8_t* d_keys, size_t key_cap, uint64_t* d_key_off,
                       uint32_t* d_key_len, uint8_t* d_vals, size_t val_cap, uint64_t* d_val_off,
                       uint32_t* d_val_len, uint32_t entry_cap, uint32_t* d_block_entry_first,
                       uint8_t* d_block_status, uint32_t* blocks_done, uint32_t* next_block,
                       int* at_end, uint8_t* index_status, uint64_t* needed, void* stream) {
  if (!d_block_status) return fail(LGS_EINVAL, "NULL argument");
  const ScanIo io{true, start, start_len, has_start, first_block, max_blocks, d_keys, key_cap,
                  d_key_off, d_key_len, d_vals, val_cap, d_val_off, d_val_len, entry_cap,
                  d_block_entry_first, d_block_status, blocks_done, next_block, at_end,
                  index_status, needed};
  return table_scan(table, verify_checksums, io, (hipStream_t)stream);
}

int lgs_device_count(void) { return visible_devices(); }

int lgs_set_device(int device) {
  int count = lgs_device_count();
  if (device < 0 || device >= count)
    return fail(LGS_ENODEV, "device %d not present (%d visible)", device, count);
  t_want_device = device;
  return LGS_OK;
}

const char* lgs_last_error(void) { return t_err; }

const char* lgs_version(void) { return "lcdb_gpu_snappy 0.1 gfx950"; }

}  // extern "C"
