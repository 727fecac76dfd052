// lgs_seek.hip -- gfx950 kernels of the batched point lookup:
// ldb_blockiter_create + one ldb_blockiter_seek per query (block.c:324-451),
// and the steps of ldb_table_internal_get (table.c:314-364) around it.
//
// One lane per query.  A seek is a chain of dependent loads (each probe of
// the binary search and each entry of the scan starts where the last one
// said), so what hides the latency is the number of queries in flight, and a
// lane per query puts the most of them on a CU.  The scan never rebuilds the
// current key: it carries the length of the prefix the key shares with the
// target (and the key's byte behind it), which an entry's `shared` count
// either leaves alone or cuts back, so keys as long as the block cost no
// buffer.  Only the bytes of an internal key's tag that lie in the shared
// part are fetched by walking the restart run again (key_bytes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lgs_device.h"
#include "lgs_seek.h"

namespace lgs {

namespace {

typedef uint64_t u64_g __attribute__((aligned(1)));
using bytes_g = gptr<const uint8_t>;

__device__ __forceinline__ uint32_t ld_le32(bytes_g p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ uint64_t ld_le64(bytes_g p) { return *(gptr<const u64_g>)p; }

// Length of the common prefix of a[0, n) and b[0, n).
__device__ __forceinline__ uint32_t common_prefix(bytes_g a, bytes_g b, uint32_t n) {
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8) {
    const uint64_t x = ld_le64(a + i) ^ ld_le64(b + i);
    if (x) return i + ((uint32_t)__builtin_ctzll(x) >> 3);
  }
  for (; i < n; ++i)
    if (a[i] != b[i]) break;
  return i;
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

__device__ __forceinline__ int sign_of(uint32_t a, uint32_t b) { return a < b ? -1 : (a > b ? 1 : 0); }

// dbformat.c:206-230 on equal user keys: the larger tag sorts first.
__device__ __forceinline__ int tag_compare(uint64_t ktag, uint64_t ttag) {
  return ktag > ttag ? -1 : (ktag < ttag ? 1 : 0);
}

// Key k[0, kn) against the target t[0, tn): memcmp then length, or with
// trim = 8 ldb_ikc_compare (both at least 8 bytes).
__device__ __forceinline__ int compare_keys(bytes_g k, uint32_t kn, bytes_g t, uint32_t tn,
                                            uint32_t trim) {
  const uint32_t ku = kn - trim, tu = tn - trim;
  const uint32_t c = ku < tu ? ku : tu;
  const uint32_t m = common_prefix(k, t, c);
  if (m < c) return sign_of(k[m], t[m]);
  if (ku != tu) return sign_of(ku, tu);
  return trim ? tag_compare(ld_le64(k + ku), ld_le64(t + tu)) : 0;
}

// Bytes [pos, pos + 8) of the key of the entry at `entry`, whose restart run
// starts at `from`: every entry of the run up to it puts its delta at
// [shared, shared + non_shared) of the key (block.c:278-279).  The entries
// have been decoded once already, so they decode.
__device__ uint64_t key_bytes(bytes_g blk, uint32_t from, uint32_t entry, uint32_t limit,
                              uint32_t pos) {
  uint64_t r = 0;
  for (uint32_t at = from; at <= entry;) {
    Entry e;
    if (!decode_entry(blk, at, limit, &e)) break;
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t x = pos + j;
      if (x >= e.shared && x - e.shared < e.non_shared)
        r = (r & ~(0xffull << (8 * j))) | ((uint64_t)blk[e.key_at + (x - e.shared)] << (8 * j));
    }
    at = e.key_at + e.non_shared + e.value_len;
  }
  return r;
}

// The key of the entry at `entry` (length klen), its first min(klen, cap)
// bytes into out.
__device__ void write_key(bytes_g blk, uint32_t from, uint32_t entry, uint32_t limit,
                          uint32_t klen, gptr<uint8_t> out, uint32_t cap) {
  const uint32_t end = klen < cap ? klen : cap;
  for (uint32_t at = from; at <= entry;) {
    Entry e;
    if (!decode_entry(blk, at, limit, &e)) break;
    const uint32_t hi = e.non_shared < end - (e.shared < end ? e.shared : end)
                            ? e.non_shared : end - (e.shared < end ? e.shared : end);
    for (uint32_t j = 0; j < hi; ++j) out[e.shared + j] = blk[e.key_at + j];
    at = e.key_at + e.non_shared + e.value_len;
  }
}

__device__ __forceinline__ uint32_t restart_array(uint32_t len, uint32_t nr) {
  return len - (1 + nr) * 4;
}

__global__ __launch_bounds__(256) void block_seek_kernel(SeekArgs a) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= a.nq) return;
  uint32_t st = kStOk, pos = kNoEntry, fklen = 0, vpos = 0, vlen = 0, from = 0;
  const uint32_t b = a.qblock ? a.qblock[q] : 0;
  const uint32_t trim = a.internal ? 8u : 0u;
  do {
    if (b >= a.nblocks) break;                            // no block: an empty iterator
    if (a.block_status && a.block_status[b] != kStOk) {   // an error iterator
      st = a.block_status[b];
      break;
    }
    const bytes_g blk = to_global(a.blocks) + a.block_off[b];
    const uint32_t len = a.block_len[b];
    if (len < 4) {                                        // block.c:58-59, 434-435
      st = kStCorrupt;
      break;
    }
    const uint32_t nr = ld_le32(blk + (len - 4));
    if (nr > (len - 4) / 4) {                             // block.c:61-65
      st = kStCorrupt;
      break;
    }
    if (nr == 0) break;                                   // block.c:439-440
    const uint32_t restarts = restart_array(len, nr);
    const bytes_g t = to_global(a.keys) + a.key_off[q];
    const uint32_t tn = a.key_len[q];
    if (tn < trim) {                                      // block.c:329-332
      st = kStCorrupt;
      break;
    }
    // block.c:357-389.
    uint32_t left = 0, right = nr - 1;
    bool bad = false;
    while (left < right) {
      const uint32_t mid = (left + right + 1) / 2;
      uint32_t off = ld_le32(blk + restarts + 4 * mid);
      if (off > restarts) off = restarts;                 // get_restart_point (:159-170)
      Entry e;
      if (!decode_entry(blk, off, restarts, &e) || e.shared != 0 || e.non_shared < trim) {
        bad = true;
        break;
      }
      if (compare_keys(blk + e.key_at, e.non_shared, t, tn, trim) < 0)
        left = mid;
      else
        right = mid - 1;
    }
    if (bad) {
      st = kStCorrupt;
      break;
    }
    from = ld_le32(blk + restarts + 4 * left);
    if (from > restarts) from = restarts;
    // block.c:402-408.  klen: the previous key's length; pre: the prefix it
    // shares with the target's user key, at most either's length; kb: its
    // byte behind that prefix, if it has one.  Every key passed so far
    // compared below the target.
    const uint32_t tu = tn - trim;
    uint32_t cur = from, klen = 0, pre = 0, kb = 0;
    for (;;) {
      if (cur >= restarts) break;                         // block.c:258-263
      Entry e;
      if (!decode_entry(blk, cur, restarts, &e) || klen < e.shared ||
          (uint64_t)e.shared + e.non_shared < trim) {     // block.c:266-276
        st = kStCorrupt;
        break;
      }
      const bytes_g delta = blk + e.key_at;
      klen = e.shared + e.non_shared;
      if (e.shared <= pre) {
        const uint32_t room = tu - e.shared;
        const uint32_t c = e.non_shared < room ? e.non_shared : room;
        const uint32_t m = common_prefix(delta, t + e.shared, c);
        pre = e.shared + m;
        if (m < e.non_shared) kb = delta[m];
      }
      // else: the key keeps the previous key's bytes through [pre], so pre
      // and kb stand.
      const uint32_t ku = klen - trim;
      const uint32_t c = ku < tu ? ku : tu;
      int cmp;
      if (pre < c) {
        cmp = sign_of(kb, t[pre]);
      } else if (ku != tu) {
        cmp = sign_of(ku, tu);
      } else if (trim) {
        const uint64_t ktag = ku >= e.shared ? ld_le64(delta + (ku - e.shared))
                                             : key_bytes(blk, from, cur, restarts, ku);
        cmp = tag_compare(ktag, ld_le64(t + tu));
      } else {
        cmp = 0;
      }
      if (cmp >= 0) {
        pos = cur;
        fklen = klen;
        vpos = e.key_at + e.non_shared;
        vlen = e.value_len;
        break;
      }
      cur = e.key_at + e.non_shared + e.value_len;
    }
    if (pos != kNoEntry && a.key_out)
      write_key(blk, from, pos, restarts, fklen, to_global(a.key_out) + a.key_out_off[q],
                a.key_out_cap[q]);
  } while (false);
  a.entry_pos[q] = pos;
  a.found_key_len[q] = fklen;
  a.val_pos[q] = vpos;
  a.val_len[q] = vlen;
  a.status[q] = (uint8_t)st;
  a.restart_pos[q] = from;
}

__global__ __launch_bounds__(256) void get_handles_kernel(
    const uint8_t* __restrict__ index_block, const uint32_t* __restrict__ entry_pos,
    const uint32_t* __restrict__ val_pos, const uint32_t* __restrict__ val_len, uint32_t nq,
    uint64_t* __restrict__ hoff, uint64_t* __restrict__ hsize, uint8_t* __restrict__ state) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  uint64_t o = 0, s = 0;
  uint8_t r = 0;
  if (entry_pos[q] != kNoEntry) {
    const bytes_g p = to_global(index_block);
    uint32_t at = val_pos[q];
    const uint32_t limit = at + val_len[q];
    r = varint64(p, &at, limit, &o) && varint64(p, &at, limit, &s) ? 1 : 2;
  }
  hoff[q] = o;
  hsize[q] = s;
  state[q] = r;
}

__global__ __launch_bounds__(256) void get_lens_kernel(
    const uint32_t* __restrict__ qblock, const uint8_t* __restrict__ pre,
    const uint32_t* __restrict__ entry_pos, const uint32_t* __restrict__ found_key_len,
    const uint32_t* __restrict__ val_len, const uint8_t* __restrict__ seek_status, uint32_t nq,
    uint8_t* __restrict__ called, uint8_t* __restrict__ status, uint32_t* __restrict__ out_len) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  if (qblock[q] == kNoBlock) {
    called[q] = 0;
    status[q] = pre[q];
    out_len[q] = 0;
    return;
  }
  const bool hit = entry_pos[q] != kNoEntry;
  called[q] = hit ? 1 : 0;
  status[q] = seek_status[q];
  out_len[q] = hit ? found_key_len[q] + val_len[q] : 0;
}

__global__ __launch_bounds__(256) void get_gather_kernel(GatherArgs a) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q > a.nq) return;
  if (q == a.nq) {
    a.out_val_off[q] = a.out_key_off[q];
    return;
  }
  const uint64_t ko = a.out_key_off[q];
  uint8_t verdict = kGetNotFound;
  uint64_t src = 0;
  uint32_t vn = 0, kn = 0;
  if (a.called[q]) {
    const uint32_t b = a.qblock[q];
    const bytes_g blk = to_global(a.blocks) + a.block_off[b];
    kn = a.found_key_len[q];
    vn = a.val_len[q];
    src = a.block_off[b] + a.val_pos[q];
    const gptr<uint8_t> key = to_global(a.out) + ko;
    // The entries up to the found one end before its value: a limit that
    // lets them decode again.
    write_key(blk, a.restart_pos[q], a.entry_pos[q], a.val_pos[q] + vn, kn, key, kn);
    if (a.verdict) {                                      // save_value, version_set.c:373-388
      const bytes_g t = to_global(a.keys) + a.key_off[q];
      const uint32_t tn = a.key_len[q];
      const bytes_g k = (bytes_g)key;
      if (kn < 8 || k[kn - 8] > 1) {
        verdict = kGetCorrupt;
      } else if (tn >= 8 && kn == tn && common_prefix(k, t, kn - 8) == kn - 8) {
        verdict = k[kn - 8] == 1 ? kGetFound : kGetDeleted;
      }
    }
  }
  a.out_val_off[q] = ko + kn;
  a.val_src[q] = src;
  a.val_n[q] = vn;
  if (a.verdict) a.verdict[q] = verdict;
}

// ---- the opened table's Get: de-duplication on the device ----------------
//
// All a lane per item over coalesced 1-, 4- and 8-byte arrays; only
// block_plan_kernel's two loads per block (type byte, size header) are
// scattered.

// table.c:345-352 before the block read, as lgs_table_get_host's host loop
// has it: pre[q] for a query that reads no block, and for a live one (a
// handle, and no filter or a filter match) a mark on the index entry it
// found.  qblock[q] holds that entry's offset until qblock_kernel.
__global__ __launch_bounds__(256) void live_mark_kernel(
    const uint8_t* __restrict__ state, const uint8_t* __restrict__ match,
    const uint8_t* __restrict__ seek_status, const uint32_t* __restrict__ entry_pos, uint32_t nq,
    uint32_t index_len, uint8_t* __restrict__ pre, uint32_t* __restrict__ qblock,
    uint32_t* __restrict__ mark) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const uint32_t st = state[q], pos = entry_pos[q];
  uint32_t p = kStOk;
  bool live = false;
  if (st == 0) {
    p = seek_status[q];                                    // the index iterator's status
  } else if (st == 2) {
    p = kStCorrupt;                                        // table.c:244-245
  } else {
    live = (!match || match[q]) && pos < index_len;
  }
  pre[q] = (uint8_t)p;
  qblock[q] = live ? pos : kNoBlock;
  if (live) mark[pos] = 1u;
}

// rank: the exclusive scan of the marks, so a marked entry's rank is its
// block's number, in file order.  Every query of a block writes the block's
// handle; they all found the same entry, so they write the same two words.
__global__ __launch_bounds__(256) void qblock_kernel(
    const uint64_t* __restrict__ rank, const uint64_t* __restrict__ hoff,
    const uint64_t* __restrict__ hsize, uint32_t nq, uint32_t* __restrict__ qblock,
    uint64_t* __restrict__ b_off, uint64_t* __restrict__ b_size) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const uint32_t pos = qblock[q];
  if (pos == kNoBlock) return;
  const uint32_t b = (uint32_t)rank[pos];
  qblock[q] = b;
  b_off[b] = hoff[q];
  b_size[b] = hsize[q];
}

// plan_handle (lgs_api.cpp) per distinct block of a resident image: the room
// its contents take, 0 for a handle outside the file.  info: {nb (read),
// += the 16-aligned rooms, max= the rooms, |= 1 for a block of 2^31 bytes
// or more}, one atomic each per workgroup.
__global__ __launch_bounds__(256) void block_plan_kernel(
    const uint8_t* __restrict__ file, uint64_t file_len, const uint64_t* __restrict__ b_off,
    const uint64_t* __restrict__ b_size, uint32_t bound, uint32_t* __restrict__ out_cap,
    uint32_t* __restrict__ room, uint64_t* __restrict__ info) {
  __shared__ uint64_t s_sum;
  __shared__ uint32_t s_max, s_err;
  if (threadIdx.x == 0) {
    s_sum = 0;
    s_max = 0;
    s_err = 0;
  }
  __syncthreads();
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  const uint64_t nb = info[0];
  if (j < bound && j < nb) {
    const uint64_t off = b_off[j], size = b_size[j];
    const bool in_file = size <= ~0ull - kTrailerBytes && off <= file_len &&
                         file_len - off >= size + kTrailerBytes;
    uint32_t cap = 0;
    if (in_file && size > 0x7fffffffull) {
      atomicOr(&s_err, 1u);
    } else if (in_file) {
      const bytes_g p = to_global(file) + off;
      cap = (uint32_t)size;
      if (p[size] == 1) {                                  // LGS_SNAPPY_COMPRESSION
        uint32_t want = 0, at = 0;
        const uint64_t most = 32 * size + 64;
        cap = varint32(p, &at, (uint32_t)size, &want) ? want : 0u;
        if (cap > most) cap = (uint32_t)most;
        if (cap > kMaxRoom) cap = kMaxRoom;
      }
    }
    const uint32_t r16 = (cap + 15u) & ~15u;
    out_cap[j] = cap;
    room[j] = r16;
    atomicAdd((unsigned long long*)&s_sum, (unsigned long long)r16);
    atomicMax(&s_max, cap);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_sum) atomicAdd((unsigned long long*)&info[1], (unsigned long long)s_sum);
    if (s_max) atomicMax((unsigned long long*)&info[2], (unsigned long long)s_max);
    if (s_err) atomicOr((unsigned long long*)&info[3], 1ull);
  }
}

// Every query's answer for a table that did not open.
__global__ __launch_bounds__(256) void get_fail_kernel(uint32_t nq, uint32_t st,
                                                       uint8_t* __restrict__ called,
                                                       uint8_t* __restrict__ status,
                                                       uint8_t* __restrict__ verdict,
                                                       uint64_t* __restrict__ out_key_off,
                                                       uint64_t* __restrict__ out_val_off) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q > nq) return;
  out_key_off[q] = 0;
  out_val_off[q] = 0;
  if (q == nq) return;
  called[q] = 0;
  status[q] = (uint8_t)st;
  if (verdict) verdict[q] = kGetNotFound;
}

// The room's cap stands for "corrupted compressed block contents"
// (format.c:247-251).
__global__ __launch_bounds__(256) void nospace_is_corrupt_kernel(uint8_t* __restrict__ status,
                                                                 uint32_t nq) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q < nq && status[q] == kStNoSpace) status[q] = (uint8_t)kStCorrupt;
}

}  // namespace

hipError_t launch_live_mark(const uint8_t* state, const uint8_t* match, const uint8_t* seek_status,
                            const uint32_t* entry_pos, uint32_t nq, uint32_t index_len,
                            uint8_t* pre, uint32_t* qblock, uint32_t* mark, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(live_mark_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, state, match,
                     seek_status, entry_pos, nq, index_len, pre, qblock, mark);
  return hipGetLastError();
}

hipError_t launch_qblock(const uint64_t* rank, const uint64_t* hoff, const uint64_t* hsize,
                         uint32_t nq, uint32_t* qblock, uint64_t* b_off, uint64_t* b_size,
                         hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(qblock_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, rank, hoff, hsize, nq,
                     qblock, b_off, b_size);
  return hipGetLastError();
}

hipError_t launch_block_plan(const uint8_t* file, uint64_t file_len, const uint64_t* b_off,
                             const uint64_t* b_size, uint32_t bound, uint32_t* out_cap,
                             uint32_t* room, uint64_t* info, hipStream_t s) {
  if (bound == 0) return hipSuccess;
  hipLaunchKernelGGL(block_plan_kernel, dim3((bound + 255) / 256), dim3(256), 0, s, file, file_len,
                     b_off, b_size, bound, out_cap, room, info);
  return hipGetLastError();
}

hipError_t launch_get_fail(uint32_t nq, uint8_t st, uint8_t* called, uint8_t* status,
                           uint8_t* verdict, uint64_t* out_key_off, uint64_t* out_val_off,
                           hipStream_t s) {
  hipLaunchKernelGGL(get_fail_kernel, dim3((nq + 256) / 256), dim3(256), 0, s, nq, (uint32_t)st,
                     called, status, verdict, out_key_off, out_val_off);
  return hipGetLastError();
}

hipError_t launch_nospace_is_corrupt(uint8_t* status, uint32_t nq, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(nospace_is_corrupt_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, status, nq);
  return hipGetLastError();
}

hipError_t launch_block_seek(const SeekArgs& a, hipStream_t s) {
  if (a.nq == 0) return hipSuccess;
  hipLaunchKernelGGL(block_seek_kernel, dim3((a.nq + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_get_handles(const uint8_t* index_block, const uint32_t* entry_pos,
                              const uint32_t* val_pos, const uint32_t* val_len, uint32_t nq,
                              uint64_t* hoff, uint64_t* hsize, uint8_t* state, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(get_handles_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, index_block,
                     entry_pos, val_pos, val_len, nq, hoff, hsize, state);
  return hipGetLastError();
}

hipError_t launch_get_lens(const uint32_t* qblock, const uint8_t* pre, const uint32_t* entry_pos,
                           const uint32_t* found_key_len, const uint32_t* val_len,
                           const uint8_t* seek_status, uint32_t nq, uint8_t* called,
                           uint8_t* status, uint32_t* out_len, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(get_lens_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, qblock, pre,
                     entry_pos, found_key_len, val_len, seek_status, nq, called, status, out_len);
  return hipGetLastError();
}

hipError_t launch_get_gather(const GatherArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(get_gather_kernel, dim3((a.nq + 256) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace lgs
