// lgs_merge.hip -- gfx950 kernels of the merge of sorted runs:
// ldb_mergeiter_first + _next until invalid (merger.c:107-128, 155-194) over
// up to 64 runs in the block builder's input layout, and the drop loop of
// ldb_do_compaction_work (db_impl.c:1363-1397) over the merged order.
//
// Nothing here moves key bytes until the last kernel.  Every input entry gets
// a number (the runs one after the other) and a 64-bit word: the first eight
// bytes of its comparable key, big-endian, zero padded.  ceil(log2 k) passes
// then merge adjacent pairs of run groups as (word, number) pairs through two
// ping-pong arrays, a lane per entry: an entry of the left group lands at its
// own rank plus the lower bound of its key in the right group, one of the
// right group at its rank plus the upper bound in the left one.  That is a
// stable two-way merge, and adjacent pairing keeps the lowest-numbered run
// first among equal keys, as find_smallest's strict `<` does.  A compare looks
// at the words, and only where they agree at the bytes from offset 8, the
// lengths and (internal keys) the tag.
//
// The drop rule needs entry i and entry i - 1 of the merged order only, so it
// is a lane per entry too, which also notes where each entry's bytes lie;
// three prefix scans (launch_scan) turn the keep flags and the kept lengths
// into output positions, and the emit copies keys and values with 16 lanes
// per entry, as lgs_scan.hip's, from loads that do not depend on one another.
//
// Inside a version (tools/sim_compact_version.py) the plan also
// takes the files of the levels below the output: the drop rule asks
// ldb_compaction_is_base_level_for_key per entry, a bisection per level, and
// ldb_compaction_should_stop_before's stops over the pre-drop order are a
// bisection per entry and a chain from entry 0 by pointer doubling, folded
// onto the kept entries as forced file starts for lgs_block.hip's cut.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lgs_device.h"
#include "lgs_merge.h"
#include "lgs_span.h"

namespace lgs {

namespace {

constexpr uint32_t kGroup = kSpanLanes;      // lanes per entry in the copy (copy_span, lgs_span.h)
constexpr uint32_t kPutRuns = 16;            // runs per runs_put_kernel launch
constexpr uint64_t kMaxSequence = (1ull << 56) - 1;   // LDB_MAX_SEQUENCE, dbformat.h
constexpr uint32_t kTypeDeletion = 0;        // LDB_TYPE_DELETION
constexpr uint32_t kTypeValue = 1;           // LDB_TYPE_VALUE: above it ldb_pkey_import fails

typedef uint64_t u64_a1 __attribute__((aligned(1)));
using bytes_g = gptr<const uint8_t>;

struct RunChunk {
  MergeRun r[kPutRuns];
};

// The run table goes to the device as kernel arguments, so that no host
// buffer has to outlive an asynchronous copy.
__global__ void runs_put_kernel(RunChunk c, uint32_t base, uint32_t count, uint32_t nruns,
                                uint32_t n_total, MergeRun* __restrict__ table,
                                uint32_t* __restrict__ first, uint64_t* __restrict__ counts) {
  const uint32_t t = threadIdx.x;
  if (t < count) {
    table[base + t] = c.r[t];
    first[base + t] = c.r[t].first;
  }
  if (base + count >= nruns && t >= nruns && t <= kMergeMaxRuns) first[t] = n_total;
  if (counts && base == 0 && t == 0) counts[5] = ~0ull;
}

// The run that holds entry number (or, in a pass, position) e < n_total: the
// last run r with first[r] <= e, which is never an empty one.
__device__ __forceinline__ uint32_t run_of(const uint32_t* __restrict__ first, uint32_t nruns,
                                           uint32_t e) {
  uint32_t lo = 0, hi = nruns;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (first[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

struct KeyRef {
  bytes_g p;
  uint32_t len, ulen;    // ulen: the comparable bytes (internal keys: without the tag)
};

__device__ __forceinline__ KeyRef key_ref(const MergeRun& r, uint32_t i, uint32_t internal) {
  const uint32_t len = r.key_len[i];
  return KeyRef{to_global(r.keys) + r.key_off[i], len,
                internal ? (len >= 8 ? len - 8 : 0u) : len};
}

__device__ __forceinline__ KeyRef key_of(const MergeRun* __restrict__ table,
                                         const uint32_t* __restrict__ first,
                                         const uint8_t* __restrict__ erun, uint32_t e,
                                         uint32_t internal) {
  const uint32_t r = erun[e];
  return key_ref(table[r], e - first[r], internal);
}

// The first min(len, 8) bytes at p as a big-endian word, zero padded.  Reads
// 8 bytes whatever len is (the buffers' 16 spare bytes).
__device__ __forceinline__ uint64_t word_at(bytes_g p, uint32_t len) {
  const uint64_t w = __builtin_bswap64(*(gptr<const u64_a1>)p);
  if (len >= 8) return w;
  return len ? w & (~0ull << (8 * (8 - len))) : 0;
}

__device__ __forceinline__ uint64_t tag_of(const KeyRef& k) {       // dbformat.c:94-98
  return k.len >= 8 ? *(gptr<const u64_a1>)(k.p + k.ulen) : 0;
}

// The compare of two keys whose words agree: the bytes from offset 8, then
// the lengths ("ab" < "ab\0": comparator.c:44-60), then the tag, descending
// (dbformat.c:232-285).
__device__ __forceinline__ int cmp_rest(const KeyRef& a, const KeyRef& b, uint32_t internal) {
  const uint32_t m = a.ulen < b.ulen ? a.ulen : b.ulen;
  for (uint32_t o = 8; o < m; o += 8) {
    const uint64_t wa = word_at(a.p + o, m - o), wb = word_at(b.p + o, m - o);
    if (wa != wb) return wa < wb ? -1 : 1;
  }
  if (a.ulen != b.ulen) return a.ulen < b.ulen ? -1 : 1;
  if (internal) {
    const uint64_t ta = tag_of(a), tb = tag_of(b);
    if (ta != tb) return ta > tb ? -1 : 1;
  }
  return 0;
}

__device__ __forceinline__ int cmp_keys(const KeyRef& a, const KeyRef& b, uint32_t internal) {
  const uint64_t wa = word_at(a.p, a.ulen), wb = word_at(b.p, b.ulen);
  if (wa != wb) return wa < wb ? -1 : 1;
  return cmp_rest(a, b, internal);
}

// ---- the levels below the output ---------------------------

__device__ __forceinline__ KeyRef file_key(const VersionDev& v, uint32_t f, bool largest) {
  const VersionFile& m = v.files[f];
  const uint32_t len = largest ? m.l_len : m.s_len;
  return KeyRef{to_global(v.keys) + (largest ? m.l_off : m.s_off), len, len - 8};
}

// ldb_compaction_is_base_level_for_key (version_set.c:2289-2321) as a pure
// function of the user key: per level the first file whose largest user key
// is >= the key, by bisection, must not exist or must start behind the key.
__device__ __forceinline__ bool base_level(const VersionDev& v, const KeyRef& k) {
  for (uint32_t lv = 0; lv < v.nlevels; ++lv) {
    uint32_t lo = v.first[lv];
    const uint32_t end = v.first[lv + 1];
    uint32_t hi = end;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (cmp_keys(file_key(v, mid, true), k, 0) >= 0) hi = mid; else lo = mid + 1;
    }
    if (lo < end && cmp_keys(file_key(v, lo, false), k, 0) <= 0) return false;
  }
  return true;
}

// Per input entry: its word, its number and its run; and the preconditions by
// a compare with the entry before it in its run.
__global__ __launch_bounds__(256) void words_kernel(const MergeRun* __restrict__ table,
                                                    const uint32_t* __restrict__ first,
                                                    uint32_t nruns, uint32_t n, uint32_t internal,
                                                    uint64_t* __restrict__ kw,
                                                    uint32_t* __restrict__ idx,
                                                    uint8_t* __restrict__ erun,
                                                    uint64_t* __restrict__ counts) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const uint32_t r = run_of(first, nruns, e);
  const uint32_t i = e - first[r];
  const MergeRun& run = table[r];
  const KeyRef k = key_ref(run, i, internal);
  const uint64_t w = word_at(k.p, k.ulen);
  kw[e] = w;
  idx[e] = e;
  erun[e] = (uint8_t)r;
  bool bad = internal && k.len < 8;
  if (!bad && i > 0) {
    const KeyRef q = key_ref(run, i - 1, internal);
    const uint64_t wq = word_at(q.p, q.ulen);
    bad = wq > w || (wq == w && cmp_rest(q, k, internal) > 0);
  }
  if (bad) atomicMin((unsigned long long*)&counts[5], (unsigned long long)r);
}

// One two-way pass: groups of w runs, pair g = groups 2g and 2g + 1.
__global__ __launch_bounds__(256) void merge_pass_kernel(
    const MergeRun* __restrict__ table, const uint32_t* __restrict__ first,
    const uint8_t* __restrict__ erun, uint32_t nruns, uint32_t n, uint32_t internal, uint32_t w,
    const uint64_t* __restrict__ kw_in, const uint32_t* __restrict__ idx_in,
    uint64_t* __restrict__ kw_out, uint32_t* __restrict__ idx_out) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t r0 = run_of(first, nruns, p) / (2 * w) * (2 * w);
  const uint32_t rm = r0 + w < nruns ? r0 + w : nruns, rh = r0 + 2 * w < nruns ? r0 + 2 * w : nruns;
  const uint32_t lo = first[r0], mid = first[rm], hi = first[rh];
  const uint64_t key = kw_in[p];
  const uint32_t e = idx_in[p];
  const bool left = p < mid;
  // left: how many of the right group are < key; right: how many of the left
  // group are <= key.
  uint32_t a = left ? mid : lo, b = left ? hi : mid;
  KeyRef mine{nullptr, 0, 0};
  bool have = false;
  while (a < b) {
    const uint32_t m = a + (b - a) / 2;
    const uint64_t wm = kw_in[m];
    int c = wm < key ? -1 : wm > key ? 1 : 0;
    if (c == 0) {
      if (!have) {
        mine = key_of(table, first, erun, e, internal);
        have = true;
      }
      c = cmp_rest(key_of(table, first, erun, idx_in[m], internal), mine, internal);
    }
    if (left ? c < 0 : c <= 0) a = m + 1; else b = m;
  }
  const uint32_t dst = p + a - mid;      // left: p + (a - mid); right: lo + (p - mid) + (a - lo)
  kw_out[dst] = key;
  idx_out[dst] = e;
}

// Over the final order: the drop flag of position j from entries j and j - 1
// (db_impl.c:1363-1397), and the kept lengths.  An entry whose type byte is
// above 1 fails ldb_pkey_import: it is kept, and the entry behind it starts
// over at kMaxSequence.  kVersion: base_level(v, key) stands where
// rule.drop_deletions does.
template <bool kVersion>
__global__ __launch_bounds__(256) void neighbour_kernel(
    const MergeRun* __restrict__ table, const uint32_t* __restrict__ first,
    const uint8_t* __restrict__ erun, uint32_t n, MergeRule rule, VersionDev v,
    const uint64_t* __restrict__ kw, const uint32_t* __restrict__ idx,
    uint32_t* __restrict__ keep, uint32_t* __restrict__ klen, uint32_t* __restrict__ vlen,
    uint64_t* __restrict__ ksrc, uint64_t* __restrict__ vsrc, uint64_t* __restrict__ from,
    uint64_t* __restrict__ counts) {
  __shared__ unsigned long long s_max;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) {
    const uint32_t e = idx[j], r = erun[e], i = e - first[r];
    const MergeRun& run = table[r];
    const KeyRef k = key_ref(run, i, rule.internal);
    bool drop = false;
    if (rule.drop) {
      const uint64_t tag = tag_of(k);
      uint64_t last = kMaxSequence;                          // :1367, :1373
      if (j > 0 && kw[j - 1] == kw[j]) {
        const KeyRef q = key_of(table, first, erun, idx[j - 1], 1);
        const uint64_t qtag = tag_of(q);
        // The same user key, and ldb_pkey_import took the entry before: :1396.
        // Behind an unparsable one lcdb has no current user key (:1365-1367).
        if ((uint32_t)(qtag & 0xff) <= kTypeValue && cmp_rest(q, k, 0) == 0) last = qtag >> 8;
      }
      drop = (uint32_t)(tag & 0xff) <= kTypeValue &&         // else "do not hide error keys", :1363
             (last <= rule.smallest_snapshot ||              // (A), :1376
              ((uint32_t)(tag & 0xff) == kTypeDeletion && (tag >> 8) <= rule.smallest_snapshot &&
               (kVersion ? base_level(v, k) : rule.drop_deletions != 0)));   // :1379-1382
    }
    keep[j] = drop ? 0u : 1u;
    klen[j] = drop ? 0u : k.len;
    vlen[j] = drop ? 0u : run.val_len[i];
    // Where the emit finds the bytes, so that its loads per entry do not
    // depend on one another.
    ksrc[j] = (uint64_t)(uintptr_t)(run.keys + run.key_off[i]);
    vsrc[j] = (uint64_t)(uintptr_t)(run.vals + run.val_off[i]);
    from[j] = (uint64_t)i << 32 | r;
    if (!drop) atomicMax(&s_max, (unsigned long long)k.len);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_max) atomicMax((unsigned long long*)&counts[3], s_max);
}

__global__ void plan_finish_kernel(const uint64_t* __restrict__ tot, uint32_t n,
                                   uint64_t* __restrict__ counts) {
  counts[0] = tot[0];
  counts[1] = tot[1];
  counts[2] = tot[2];
  counts[4] = n - tot[0];
}

// ---- ldb_compaction_should_stop_before over the final order (§4.10) -------
// overlapped_bytes before position i is pg[i] less pg at the last stop (or at
// position 0, whose passed files cost nothing: seen_key, version_set.c:2337),
// so the stop behind i is a search and the stops are a chain from position 0.

// pg[j] = P[files of level + 2 whose largest key is < key j], by the raw tag.
__global__ __launch_bounds__(256) void passed_kernel(
    const MergeRun* __restrict__ table, const uint32_t* __restrict__ first,
    const uint8_t* __restrict__ erun, uint32_t n, VersionDev v, const uint32_t* __restrict__ idx,
    uint64_t* __restrict__ pg, uint32_t* __restrict__ mark) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const KeyRef k = key_of(table, first, erun, idx[j], 1);
  uint32_t lo = 0, hi = v.first[1];
  while (lo < hi) {                                  // version_set.c:2331-2335
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cmp_keys(file_key(v, mid, true), k, 1) >= 0) hi = mid; else lo = mid + 1;
  }
  pg[j] = v.P[lo];
  mark[j] = j == 0 ? 1u : 0u;
}

// The first position behind i whose overlap since i is over the limit; n when
// there is none.  pg does not decrease.
__global__ __launch_bounds__(256) void stop_next_kernel(const uint64_t* __restrict__ pg,
                                                        uint64_t limit,
                                                        uint32_t* __restrict__ next, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t base = pg[i];
  uint32_t lo = i + 1, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pg[mid] - base > limit) hi = mid; else lo = mid + 1;   // :2343
  }
  next[i] = lo;
}

// One round of pointer doubling (lgs_block.hip's jump_kernel).
__global__ __launch_bounds__(256) void stop_jump_kernel(uint32_t* mark,
                                                        const uint32_t* __restrict__ jin,
                                                        uint32_t* __restrict__ jout, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = jin[i];
  if (j < n && mark[i]) mark[j] = 1u;
  jout[i] = j < n ? jin[j] : n;
}

// Per kept entry: the stops at positions up to and with its own (sid: the
// exclusive scan of the marks, position 0's cleared).
__global__ __launch_bounds__(256) void stop_fold_kernel(
    uint32_t n, const uint32_t* __restrict__ keep, const uint64_t* __restrict__ pos,
    const uint32_t* __restrict__ mark, const uint64_t* __restrict__ sid,
    uint32_t* __restrict__ cnt) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n || !keep[j]) return;
  cnt[pos[j]] = (uint32_t)sid[j] + mark[j];
}

// Kept entry k > 0 starts a file when a stop lies behind kept entry k - 1 and
// not behind k itself: the builder is open then (db_impl.c:1354-1360).  A stop
// up to the first kept entry finds no builder.
__global__ __launch_bounds__(256) void forced_kernel(const uint64_t* __restrict__ tot,
                                                     const uint32_t* __restrict__ cnt,
                                                     uint32_t* __restrict__ forced,
                                                     uint64_t* __restrict__ counts) {
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k < tot[0]) {
    const uint32_t f = k > 0 && cnt[k] != cnt[k - 1] ? 1u : 0u;
    forced[k] = f;
    if (f) atomicAdd(&s_sum, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_sum)
    atomicAdd((unsigned long long*)&counts[6], (unsigned long long)s_sum);
}

__global__ __launch_bounds__(256) void merge_emit_kernel(
    uint32_t n, uint32_t n_out, const uint32_t* __restrict__ keep,
    const uint32_t* __restrict__ klen, const uint32_t* __restrict__ vlen,
    const uint64_t* __restrict__ ksrc, const uint64_t* __restrict__ vsrc,
    const uint64_t* __restrict__ from, const uint64_t* __restrict__ pos,
    const uint64_t* __restrict__ koff, const uint64_t* __restrict__ voff,
    const uint64_t* __restrict__ tot,
    uint8_t* __restrict__ keys, uint64_t* __restrict__ key_off, uint32_t* __restrict__ key_len,
    uint8_t* __restrict__ vals, uint64_t* __restrict__ val_off, uint32_t* __restrict__ val_len,
    uint32_t* __restrict__ src_run, uint32_t* __restrict__ src_index) {
  const uint32_t gl = threadIdx.x & (kGroup - 1);
  const uint32_t groups = gridDim.x * (256 / kGroup);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    key_off[n_out] = tot[1];
    val_off[n_out] = tot[2];
  }
  for (uint32_t j = blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup; j < n; j += groups) {
    const uint32_t kept = keep[j], kl = klen[j], vl = vlen[j];
    const uint64_t o = pos[j], ko = koff[j], vo = voff[j], ks = ksrc[j], vs = vsrc[j], f = from[j];
    if (!kept || o >= n_out) continue;   // never more entries than the caller has room for
    copy_span(to_global((const uint8_t*)(uintptr_t)ks), to_global(keys) + ko, kl, gl);
    copy_span(to_global((const uint8_t*)(uintptr_t)vs), to_global(vals) + vo, vl, gl);
    if (gl == 0) {
      key_off[o] = ko;
      key_len[o] = kl;
      val_off[o] = vo;
      val_len[o] = vl;
      src_run[o] = (uint32_t)f;
      src_index[o] = (uint32_t)(f >> 32);
    }
  }
}

uint32_t grid256(uint32_t n) { return (n + 255) / 256; }

void put_runs(const MergeRun* runs, uint32_t nruns, uint32_t n, const MergeScratch& w,
              uint64_t* counts, hipStream_t s) {
  uint32_t base = 0;
  do {
    RunChunk c{};
    const uint32_t count = nruns - base < kPutRuns ? nruns - base : kPutRuns;
    for (uint32_t t = 0; t < count; ++t) c.r[t] = runs[base + t];
    hipLaunchKernelGGL(runs_put_kernel, dim3(1), dim3(128), 0, s, c, base, count, nruns, n,
                       w.table, w.first, counts);
    base += count;
  } while (base < nruns);
}

// The plan; v, x: the levels below the output and the stops' scratch, or null.
hipError_t plan(const MergeRun* runs, uint32_t nruns, uint32_t n, const MergeRule& rule,
                const MergeScratch& w, const VersionDev* v, const VersionScratch* x,
                uint64_t* counts, hipStream_t s) {
  hipError_t e = hipMemsetAsync(counts, 0, 8 * kMergeCounts, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.tot, 0, 32, s)) != hipSuccess) return e;
  put_runs(runs, nruns, n, w, counts, s);
  if (n == 0) return hipGetLastError();
  hipLaunchKernelGGL(words_kernel, dim3(grid256(n)), dim3(256), 0, s, w.table, w.first, nruns, n,
                     rule.internal, w.kw[0], w.idx[0], w.erun, counts);
  // A pass over runs that are not sorted (counts[5] set) can leave places
  // unwritten: they must still hold entry numbers, whatever the scratch held.
  if (nruns > 1 && (e = hipMemsetAsync(w.idx[1], 0, 4 * (size_t)n, s)) != hipSuccess) return e;
  uint32_t at = 0;
  for (uint32_t width = 1; width < nruns; width *= 2, at ^= 1)
    hipLaunchKernelGGL(merge_pass_kernel, dim3(grid256(n)), dim3(256), 0, s, w.table, w.first,
                       w.erun, nruns, n, rule.internal, width, w.kw[at], w.idx[at], w.kw[at ^ 1],
                       w.idx[at ^ 1]);
  if (v)
    hipLaunchKernelGGL(neighbour_kernel<true>, dim3(grid256(n)), dim3(256), 0, s, w.table, w.first,
                       w.erun, n, rule, *v, w.kw[at], w.idx[at], w.keep, w.klen, w.vlen, w.ksrc,
                       w.vsrc, w.from, counts);
  else
    hipLaunchKernelGGL(neighbour_kernel<false>, dim3(grid256(n)), dim3(256), 0, s, w.table, w.first,
                       w.erun, n, rule, VersionDev{}, w.kw[at], w.idx[at], w.keep, w.klen, w.vlen,
                       w.ksrc, w.vsrc, w.from, counts);
  if ((e = launch_scan(2, nullptr, w.keep, w.part, 0, w.pos, w.tot, n, s)) != hipSuccess) return e;
  if ((e = launch_scan(2, nullptr, w.klen, w.part, 0, w.koff, w.tot + 1, n, s)) != hipSuccess)
    return e;
  if ((e = launch_scan(2, nullptr, w.vlen, w.part, 0, w.voff, w.tot + 2, n, s)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(plan_finish_kernel, dim3(1), dim3(1), 0, s, w.tot, n, counts);
  if (!v) return hipGetLastError();
  const dim3 g(grid256(n)), t(256);
  if (v->first[1] == 0)      // nothing in level + 2: overlapped_bytes stays 0
    return hipMemsetAsync(x->forced, 0, 4 * (size_t)n, s);
  hipLaunchKernelGGL(passed_kernel, g, t, 0, s, w.table, w.first, w.erun, n, *v, w.idx[at], x->pg,
                     x->mark);
  hipLaunchKernelGGL(stop_next_kernel, g, t, 0, s, x->pg, v->limit, x->next, n);
  // ceil(log2(n)) rounds reach the n-th stop of a chain of single positions.
  const uint32_t* jin = x->next;
  uint32_t* jout = x->ja;
  for (uint64_t reach = 1; reach < n; reach <<= 1) {
    hipLaunchKernelGGL(stop_jump_kernel, g, t, 0, s, x->mark, jin, jout, n);
    jin = jout;
    jout = jout == x->ja ? x->jb : x->ja;
  }
  // Position 0 is the chain's root, not a stop.
  if ((e = hipMemsetAsync(x->mark, 0, 4, s)) != hipSuccess) return e;
  if ((e = launch_scan(2, nullptr, x->mark, x->part, 0, x->sid, x->sid + n, n, s)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(stop_fold_kernel, g, t, 0, s, n, w.keep, w.pos, x->mark, x->sid, x->cnt);
  hipLaunchKernelGGL(forced_kernel, g, t, 0, s, w.tot, x->cnt, x->forced, counts);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_merge_plan(const MergeRun* runs, uint32_t nruns, uint32_t n,
                             const MergeRule& rule, const MergeScratch& w, uint64_t* counts,
                             hipStream_t s) {
  return plan(runs, nruns, n, rule, w, nullptr, nullptr, counts, s);
}

hipError_t launch_merge_plan_version(const MergeRun* runs, uint32_t nruns, uint32_t n,
                                     const MergeRule& rule, const MergeScratch& w,
                                     const VersionDev& v, const VersionScratch& x,
                                     uint64_t* counts, hipStream_t s) {
  return plan(runs, nruns, n, rule, w, &v, &x, counts, s);
}

hipError_t launch_merge_emit(uint32_t n, uint32_t n_out, const MergeScratch& w, uint8_t* keys,
                             uint64_t* key_off, uint32_t* key_len, uint8_t* vals,
                             uint64_t* val_off, uint32_t* val_len, uint32_t* src_run,
                             uint32_t* src_index, hipStream_t s) {
  const uint32_t per = 256 / kGroup;
  const uint32_t want = (n + per - 1) / per;
  hipLaunchKernelGGL(merge_emit_kernel, dim3(want < 65536u ? (want ? want : 1u) : 65536u), dim3(256),
                     0, s, n, n_out, w.keep, w.klen, w.vlen, w.ksrc, w.vsrc, w.from, w.pos, w.koff,
                     w.voff, w.tot, keys, key_off, key_len, vals, val_off, val_len, src_run,
                     src_index);
  return hipGetLastError();
}

}  // namespace lgs
