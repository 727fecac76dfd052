// lgs_scan.hip -- gfx950 kernels of the forward scan:
// ldb_blockiter_first + ldb_blockiter_next until invalid (block.c:247-296,
// 411-415) for many decoded blocks, the entries out in the layout the block
// builder takes (lgs_block.hip), and the opened table's index entry list.
//
// The header walk is a lane per block: a chain of dependent loads that only
// the number of chains in flight hides.  It runs twice, once to count and,
// behind a scan of the counts, once to write per entry where its key delta
// lies, its `shared` count and its link: the nearest earlier entry with a
// smaller `shared`.  The copy is then parallel over entries, 16 lanes each.
// A key's shared prefix comes from the block's bytes, never from another
// entry's output: bytes [shared_e, need) come from the entry e the link
// names, then need = shared_e, until need = 0.  Every step lowers `need`, so
// an entry's walk is no longer than its key, whatever the block holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lgs_device.h"
#include "lgs_scan.h"
#include "lgs_span.h"

namespace lgs {

namespace {

constexpr uint32_t kGroup = kSpanLanes;   // lanes per entry in the copy (copy_span, lgs_span.h)

using bytes_g = gptr<const uint8_t>;

__device__ __forceinline__ uint32_t ld_le32(bytes_g p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// coding.h:170-204 inside blk[at, limit).
__device__ __forceinline__ bool varint32(bytes_g blk, uint32_t* at, uint32_t limit, uint32_t* z) {
  uint32_t r = 0, p = *at;
  for (uint32_t sh = 0; sh <= 28 && p < limit; sh += 7) {
    const uint32_t b = blk[p++];
    if (b & 128) {
      r |= (b & 127) << sh;
    } else {
      *z = r | (b << sh);
      *at = p;
      return true;
    }
  }
  return false;
}

// coding.h:238-260 inside p[at, limit).
__device__ __forceinline__ bool varint64(bytes_g p, uint32_t* at, uint32_t limit, uint64_t* z) {
  uint64_t r = 0;
  uint32_t i = *at;
  for (uint32_t sh = 0; sh <= 63 && i < limit; sh += 7) {
    const uint64_t b = p[i++];
    if (b & 128) {
      r |= (b & 127) << sh;
    } else {
      *z = r | (b << sh);
      *at = i;
      return true;
    }
  }
  return false;
}

struct Entry {
  uint32_t shared, non_shared, value_len, key_at;   // key_at: offset of the key delta
};

// decode_entry (block.c:86-125) at blk[at], at <= limit.
__device__ __forceinline__ bool decode_entry(bytes_g blk, uint32_t at, uint32_t limit, Entry* e) {
  if (limit - at < 3) return false;
  uint32_t s = blk[at], n = blk[at + 1], v = blk[at + 2];
  uint32_t p = at;
  if ((s | n | v) < 128) {
    p += 3;
  } else if (!varint32(blk, &p, limit, &s) || !varint32(blk, &p, limit, &n) ||
             !varint32(blk, &p, limit, &v)) {
    return false;
  }
  if ((uint64_t)(limit - p) < (uint64_t)n + v) return false;
  e->shared = s;
  e->non_shared = n;
  e->value_len = v;
  e->key_at = p;
  return true;
}

// ldb_blockiter_create's checks (block.c:58-65, 434-440): false = no walk,
// *st says why; true: *restarts = the restart array's offset.
__device__ __forceinline__ bool open_block(bytes_g blk, uint32_t len, uint32_t* st,
                                           uint32_t* restarts) {
  if (len < 4) {
    *st = kStCorrupt;
    return false;
  }
  const uint32_t nr = ld_le32(blk + (len - 4));
  if (nr > (len - 4) / 4) {
    *st = kStCorrupt;
    return false;
  }
  if (nr == 0) return false;
  *restarts = len - (1 + nr) * 4;
  return true;
}

// What one lane's walk of one block leaves in the per-entry arrays (second
// run only), all null in the first run.
struct WalkOut {
  uint32_t* src; uint32_t* shared; uint32_t* link; uint32_t* eblk; uint32_t* emeta;
  uint32_t* key_len; uint32_t* val_len;
  uint64_t wcap, ncap;   // room of the per-walked-entry and per-delivered-entry arrays
};

struct WalkSum {
  uint32_t st, walked, delivered, max_key;
  uint64_t key_bytes, val_bytes;
};

// ldb_blockiter_first + _next until invalid on block b.  kWrite: walked entry
// k goes to slot m0 + k, delivered entry k to slot i0 + k.
template <bool kWrite>
__device__ __forceinline__ WalkSum walk_block(const EntriesIn& a, uint32_t b, uint64_t m0,
                                              uint64_t i0, const WalkOut& o) {
  WalkSum r{kStOk, 0, 0, 0, 0, 0};
  if (a.block_status && a.block_status[b] != kStOk) {     // an error iterator (table.c:286-297)
    r.st = a.block_status[b];
    return r;
  }
  const bytes_g blk = to_global(a.blocks) + a.block_off[b];
  const uint32_t len = a.block_len[b];
  uint32_t restarts = 0;
  if (!open_block(blk, len, &r.st, &restarts)) return r;
  const uint32_t trim = a.internal ? 8u : 0u;
  uint32_t cur = a.walk_from ? a.walk_from[b] : kNoOffset;
  if (cur == kNoOffset) cur = ld_le32(blk + restarts);    // seek_to_restart_point(0), :172-187
  if (cur > restarts) cur = restarts;                     // get_restart_point (:159-170)
  uint32_t from = a.emit_from ? a.emit_from[b] : kNoOffset;
  if (from == kNoOffset) from = 0;
  uint32_t klen = 0;
  while (cur < restarts) {                                // block.c:258-263
    Entry e;
    if (!decode_entry(blk, cur, restarts, &e) || klen < e.shared ||
        (uint64_t)e.shared + e.non_shared < trim) {       // :266-276
      r.st = kStCorrupt;
      break;
    }
    klen = e.shared + e.non_shared;
    const bool deliver = cur >= from;
    const uint64_t m = m0 + r.walked;
    if (kWrite && m < o.wcap) {                           // (always, for a scratch sized as asked)
      o.src[m] = e.key_at;
      o.shared[m] = e.shared;
      uint32_t j = kNoLink;
      if (e.shared) {
        // The nearest earlier entry with a smaller `shared`: the first entry
        // of the walk has shared = 0, so the chain ends.  Links passed once
        // are never passed again by a later entry: linear over the block.
        j = (uint32_t)m - 1;
        while (j < o.wcap && o.shared[j] >= e.shared) j = o.link[j];
      }
      o.link[m] = j;
      const uint64_t i = i0 + r.delivered;
      if (deliver && i < o.ncap) {
        o.eblk[i] = b;
        o.emeta[i] = (uint32_t)m;
        o.key_len[i] = klen;
        o.val_len[i] = e.value_len;
      }
    }
    if (deliver) {
      ++r.delivered;
      r.key_bytes += klen;
      r.val_bytes += e.value_len;
      if (klen > r.max_key) r.max_key = klen;
    }
    ++r.walked;
    cur = e.key_at + e.non_shared + e.value_len;
  }
  return r;
}

// The totals: an LDS atomic per block, then one global atomic per workgroup
// (blocks_kernel's lesson).
__global__ __launch_bounds__(256) void entries_count_kernel(EntriesIn a, uint32_t* __restrict__ wcnt,
                                                            uint32_t* __restrict__ dcnt,
                                                            uint8_t* __restrict__ status,
                                                            uint64_t* __restrict__ counts) {
  __shared__ unsigned long long s_kb, s_vb, s_max;
  if (threadIdx.x == 0) {
    s_kb = 0;
    s_vb = 0;
    s_max = 0;
  }
  __syncthreads();
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b < a.nblocks) {
    const WalkOut none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    const WalkSum r = walk_block<false>(a, b, 0, 0, none);
    wcnt[b] = r.walked;
    dcnt[b] = r.delivered;
    status[b] = (uint8_t)r.st;
    if (r.delivered) {
      atomicAdd(&s_kb, (unsigned long long)r.key_bytes);
      atomicAdd(&s_vb, (unsigned long long)r.val_bytes);
      atomicMax(&s_max, (unsigned long long)r.max_key);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_kb) atomicAdd((unsigned long long*)&counts[1], s_kb);
    if (s_vb) atomicAdd((unsigned long long*)&counts[2], s_vb);
    if (s_max) atomicMax((unsigned long long*)&counts[3], s_max);
  }
}

__global__ __launch_bounds__(256) void entry_first_kernel(const uint64_t* __restrict__ dfirst,
                                                          const uint64_t* __restrict__ head,
                                                          uint32_t* __restrict__ entry_first,
                                                          uint64_t* __restrict__ counts,
                                                          uint32_t nblocks) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b > nblocks) return;
  if (b == nblocks) {
    entry_first[b] = (uint32_t)head[1];
    counts[0] = head[1];
    return;
  }
  entry_first[b] = (uint32_t)dfirst[b];
}

__global__ __launch_bounds__(256) void entries_walk_kernel(EntriesIn a,
                                                           const uint64_t* __restrict__ wfirst,
                                                           const uint64_t* __restrict__ dfirst,
                                                           WalkOut o) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nblocks) return;
  (void)walk_block<true>(a, b, wfirst[b], dfirst[b], o);
}

__global__ __launch_bounds__(256) void entries_copy_kernel(
    const uint8_t* __restrict__ blocks, const uint64_t* __restrict__ block_off,
    const uint32_t* __restrict__ src, const uint32_t* __restrict__ shared,
    const uint32_t* __restrict__ link, const uint32_t* __restrict__ eblk,
    const uint32_t* __restrict__ emeta, const uint64_t* __restrict__ head, uint64_t wcap,
    uint32_t n_arg,
    uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
    const uint32_t* __restrict__ key_len, uint8_t* __restrict__ vals,
    const uint64_t* __restrict__ val_off, const uint32_t* __restrict__ val_len) {
  const uint32_t gl = threadIdx.x & (kGroup - 1);
  const uint32_t groups = gridDim.x * (256 / kGroup);
  // Never more entries than the walk wrote, whatever the caller passed.
  const uint64_t have = head[1];
  const uint32_t n = n_arg < have ? n_arg : (uint32_t)have;
  for (uint32_t i = blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup; i < n; i += groups) {
    const uint32_t m = emeta[i];
    if (m >= wcap) continue;
    const bytes_g blk = to_global(blocks) + block_off[eblk[i]];
    const uint32_t sh = shared[m], at = src[m], ns = key_len[i] - sh;
    const gptr<uint8_t> key = to_global(keys) + key_off[i];
    copy_span(blk + at, key + sh, ns, gl);                               // block.c:279
    copy_span(blk + at + ns, to_global(vals) + val_off[i], val_len[i], gl);   // :281
    // block.c:278, without the previous key: entry j is the last one before
    // this that wrote bytes [shared_j, need) of the key buffer.
    uint32_t need = sh, j = m;
    while (need) {
      j = link[j];
      if (j >= wcap) break;                          // (never, for a scratch the walk filled)
      const uint32_t sj = shared[j];
      if (sj >= need) break;
      copy_span(blk + src[j], key + sj, need - sj, gl);
      need = sj;
    }
  }
}

// ---- the index entry list -------------------------------------------------

// ldb_handle_import (format.c:66-80) of the value at blk[at, at + n).
__device__ __forceinline__ void put_index_entry(const IndexList& o, uint64_t k, bytes_g blk,
                                                uint32_t pos, uint32_t vat, uint32_t vlen) {
  uint64_t off = 0, size = 0;
  uint32_t at = vat;
  const bool ok = varint64(blk, &at, vat + vlen, &off) && varint64(blk, &at, vat + vlen, &size);
  o.pos[k] = pos;
  o.hoff[k] = ok ? off : ~0ull;
  o.hsize[k] = ok ? size : 0;
  o.state[k] = ok ? 1 : 2;
}

// Lcdb writes the index block with restart interval 1 (table_builder.c:87):
// slot k's entry is then entry k of the walk.  That holds exactly when every
// slot's entry parses with shared = 0, ends where the next slot's begins, and
// the last one ends at the restart array: the walk starts at slot 0's offset
// and each entry's end is the next one's start.
__global__ __launch_bounds__(256) void index_slots_kernel(const uint8_t* __restrict__ index,
                                                          uint32_t len, uint32_t internal,
                                                          uint32_t cap, IndexList o) {
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const bytes_g blk = to_global(index);
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  uint32_t st = kStOk, restarts = 0;
  const bool open = open_block(blk, len, &st, &restarts);
  if (!open) {
    if (k == 0) {
      o.info[0] = 0;
      o.info[1] = st;
    }
    return;
  }
  const uint32_t nr = (len - restarts) / 4 - 1;
  if (k == 0) {
    o.info[0] = nr;
    o.info[1] = kStOk;
  }
  if (nr == 1 && ld_le32(blk + restarts) >= restarts) {   // the empty table's index block
    if (k == 0) o.info[0] = 0;
  } else if (k < nr) {
    const uint32_t at = ld_le32(blk + restarts + 4 * k);
    const uint32_t end = k + 1 < nr ? ld_le32(blk + restarts + 4 * (k + 1)) : restarts;
    Entry e;
    bool good = k < cap && at < restarts && end <= restarts && at < end &&
                decode_entry(blk, at, restarts, &e) && e.shared == 0 &&
                e.non_shared >= (internal ? 8u : 0u);
    if (good) good = e.key_at + e.non_shared + e.value_len == end;
    if (good)
      put_index_entry(o, k, blk, at, e.key_at + e.non_shared, e.value_len);
    else
      atomicOr(&s_bad, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_bad) atomicOr((unsigned long long*)&o.info[2], 1ull);
}

__global__ void index_walk_kernel(const uint8_t* __restrict__ index, uint32_t len,
                                  uint32_t internal, uint32_t from, uint32_t cap, IndexList o) {
  const bytes_g blk = to_global(index);
  uint32_t st = kStOk, restarts = 0, n = 0;
  if (open_block(blk, len, &st, &restarts)) {
    const uint32_t trim = internal ? 8u : 0u;
    uint32_t cur = from == kNoOffset ? ld_le32(blk + restarts) : from;
    if (cur > restarts) cur = restarts;
    uint32_t klen = from == kNoOffset ? 0u : 0xffffffffu;
    while (cur < restarts && n < cap) {
      Entry e;
      if (!decode_entry(blk, cur, restarts, &e) || klen < e.shared ||
          (uint64_t)e.shared + e.non_shared < trim) {
        st = kStCorrupt;
        break;
      }
      klen = e.shared + e.non_shared;
      put_index_entry(o, n, blk, cur, e.key_at + e.non_shared, e.value_len);
      ++n;
      cur = e.key_at + e.non_shared + e.value_len;
    }
  }
  o.info[0] = n;
  o.info[1] = st;
  o.info[2] = 0;
}

__global__ __launch_bounds__(256) void scan_status_kernel(const uint8_t* __restrict__ state,
                                                          uint8_t* __restrict__ block_status,
                                                          uint32_t nb) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nb) return;
  if (state[j] != 1 || block_status[j] == kStNoSpace) block_status[j] = (uint8_t)kStCorrupt;
}

__global__ void scan_seek_apply_kernel(const uint32_t* __restrict__ entry_pos,
                                       const uint32_t* __restrict__ restart_pos,
                                       const uint8_t* __restrict__ seek_status,
                                       uint32_t* __restrict__ walk_from,
                                       uint32_t* __restrict__ emit_from,
                                       uint8_t* __restrict__ block_status) {
  const uint32_t pos = entry_pos[0];
  if (pos == 0xffffffffu) {
    walk_from[0] = 0xfffffffeu;          // past every restart array: an invalid iterator
    emit_from[0] = 0xfffffffeu;
    if (seek_status[0] != kStOk) block_status[0] = seek_status[0];
  } else {
    walk_from[0] = restart_pos[0];
    emit_from[0] = pos;
  }
}

__global__ void plan_info_kernel(uint64_t* __restrict__ info, uint32_t nb) {
  info[0] = nb;
  info[1] = 0;
  info[2] = 0;
  info[3] = 0;
}

uint32_t grid256(uint32_t n) { return (n + 255) / 256; }

}  // namespace

hipError_t launch_entries_count(const EntriesIn& in, const EntriesScratch& w, uint32_t* entry_first,
                                uint8_t* status, uint64_t* counts, hipStream_t s) {
  hipError_t e = hipMemsetAsync(counts, 0, 8 * kEntryCounts, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.head, 0, 16, s)) != hipSuccess) return e;
  const uint32_t n = in.nblocks;
  if (n == 0) return hipMemsetAsync(entry_first, 0, 4, s);
  hipLaunchKernelGGL(entries_count_kernel, dim3(grid256(n)), dim3(256), 0, s, in, w.wcnt, w.dcnt,
                     status, counts);
  if ((e = launch_scan(2, nullptr, w.wcnt, w.part, 0, w.wfirst, w.head, n, s)) != hipSuccess)
    return e;
  if ((e = launch_scan(2, nullptr, w.dcnt, w.part, 0, w.dfirst, w.head + 1, n, s)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(entry_first_kernel, dim3(grid256(n + 1)), dim3(256), 0, s, w.dfirst, w.head,
                     entry_first, counts, n);
  return hipGetLastError();
}

hipError_t launch_entries_emit(const EntriesIn& in, const EntriesScratch& w, uint64_t wcap,
                               uint32_t n, uint8_t* keys, uint64_t* key_off, uint32_t* key_len, uint8_t* vals,
                               uint64_t* val_off, uint32_t* val_len, hipStream_t s) {
  hipError_t e;
  if (n == 0 || in.nblocks == 0) {
    if ((e = hipMemsetAsync(key_off, 0, 8, s)) != hipSuccess) return e;
    return hipMemsetAsync(val_off, 0, 8, s);
  }
  const WalkOut o{w.src, w.shared, w.link, w.eblk, w.emeta, key_len, val_len, wcap, n};
  hipLaunchKernelGGL(entries_walk_kernel, dim3(grid256(in.nblocks)), dim3(256), 0, s, in, w.wfirst,
                     w.dfirst, o);
  if ((e = launch_scan(2, nullptr, key_len, w.part, 0, key_off, key_off + n, n, s)) != hipSuccess)
    return e;
  if ((e = launch_scan(2, nullptr, val_len, w.part, 0, val_off, val_off + n, n, s)) != hipSuccess)
    return e;
  const uint32_t per = 256 / kGroup;
  const uint32_t want = (n + per - 1) / per;
  hipLaunchKernelGGL(entries_copy_kernel, dim3(want < 65536u ? want : 65536u), dim3(256), 0, s,
                     in.blocks, in.block_off, w.src, w.shared, w.link, w.eblk, w.emeta, w.head, wcap, n,
                     keys, key_off, key_len, vals, val_off, val_len);
  return hipGetLastError();
}

hipError_t launch_index_slots(const uint8_t* index, uint32_t len, uint32_t internal, uint32_t cap,
                              const IndexList& out, hipStream_t s) {
  hipError_t e = hipMemsetAsync(out.info, 0, 32, s);
  if (e != hipSuccess) return e;
  const uint32_t slots = len / 4 + 1;
  hipLaunchKernelGGL(index_slots_kernel, dim3(grid256(slots)), dim3(256), 0, s, index, len,
                     internal, cap, out);
  return hipGetLastError();
}

hipError_t launch_index_walk(const uint8_t* index, uint32_t len, uint32_t internal, uint32_t from,
                             uint32_t cap, const IndexList& out, hipStream_t s) {
  hipLaunchKernelGGL(index_walk_kernel, dim3(1), dim3(1), 0, s, index, len, internal, from, cap,
                     out);
  return hipGetLastError();
}

hipError_t launch_scan_status(const uint8_t* state, uint8_t* block_status, uint32_t nb,
                              hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(scan_status_kernel, dim3(grid256(nb)), dim3(256), 0, s, state, block_status,
                     nb);
  return hipGetLastError();
}

hipError_t launch_scan_seek_apply(const uint32_t* entry_pos, const uint32_t* restart_pos,
                                  const uint8_t* seek_status, uint32_t* walk_from,
                                  uint32_t* emit_from, uint8_t* block_status, hipStream_t s) {
  hipLaunchKernelGGL(scan_seek_apply_kernel, dim3(1), dim3(1), 0, s, entry_pos, restart_pos,
                     seek_status, walk_from, emit_from, block_status);
  return hipGetLastError();
}

hipError_t launch_plan_info(uint64_t* info, uint32_t nb, hipStream_t s) {
  hipLaunchKernelGGL(plan_info_kernel, dim3(1), dim3(1), 0, s, info, nb);
  return hipGetLastError();
}

}  // namespace lgs
