// lgs_block.hip -- lcdb's data-block builder on gfx950: sorted key/value
// entries in, finished data blocks (ldb_blockgen_finish output) and their
// index keys out, as ldb_tablegen_add (table_builder.c:215-255) produces
// them through ldb_blockgen_add / _finish (block_builder.c:91-151) with a
// flush when ldb_blockgen_size_estimate (:153-158) reaches block_size.
//
// The cut (tools/sim_block_cut.py is the same arithmetic):
//  1. per entry: lcp with the key before; sh = its size as a shared-prefix
//     entry, fu = its size at a restart point (shared = 0);
//  2. S = prefix sum of sh; C[i] = (fu[i] - sh[i]) + C[i - R], the stride-R
//     prefix (R = restart interval), by doubling passes;
//  3. the estimate of a block s..j is then O(1) and monotone in j:
//       S[j+1] - S[s] + C[s + (j-s)/R*R] - C[s-R] + 4 ((j-s)/R + 1) + 4,
//     so next[s], the entry after the block that starts at s, is a search;
//  4. the block starts are what next[] reaches from entry 0: pointer
//     doubling, a fixed number of rounds with no host read-back; a scan of
//     the marks numbers the blocks.
// The emit is a copy: every entry's place in its block is a difference of S
// and C terms, so 16 lanes per entry write its header and move its bytes,
// and the entries at restart points write the restart array.
// The index keys are the comparator's shortest separator / short successor
// (comparator.c:44-88; dbformat.c:232-285 for internal keys).
// Compaction's output files (tools/sim_table_split.py) are
// steps 3 and 4 again over the framed blocks: a file ends after the first
// block that takes it to max_output_file_size (db_impl.c:1417-1425).
// Forced starts: an entry before which compaction closed its
// output file (ldb_compaction_should_stop_before) starts a block and a file
// whatever the sizes say; both searches then stop at the first forced index
// behind their start (first_forced), and nothing else changes.
#include "lgs_block.h"
#include "lgs_device.h"

namespace lgs {
namespace {

constexpr uint32_t kNoCut = 0xffffffffu;   // index key = the block's last key, unchanged
constexpr uint32_t kGroup = 16;            // lanes per entry in the emit

typedef uint64_t u64_a1 __attribute__((aligned(1)));
typedef u32x4 u32x4_a1 __attribute__((aligned(1)));

__device__ __forceinline__ uint32_t vl(uint32_t x) {   // ldb_varint32_size (coding.h)
  return 1u + (x >= (1u << 7)) + (x >= (1u << 14)) + (x >= (1u << 21)) + (x >= (1u << 28));
}

__device__ __forceinline__ uint32_t put_varint32(gptr<uint8_t> p, uint32_t at, uint32_t v) {
  while (v >= 128u) {
    p[at++] = (uint8_t)(v | 128u);
    v >>= 7;
  }
  p[at++] = (uint8_t)v;
  return at;
}

// ---- step 1 ---------------------------------------------------------------

__global__ __launch_bounds__(256) void sizes_kernel(
    const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
    const uint32_t* __restrict__ key_len, const uint32_t* __restrict__ val_len,
    uint32_t* __restrict__ lcp, uint32_t* __restrict__ sh, uint64_t* __restrict__ c0,
    uint32_t* __restrict__ mark, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t kl = key_len[i], vlen = val_len[i];
  uint32_t l = 0;
  if (i > 0) {                                       // block_builder.c:107-110
    const uint32_t pl = key_len[i - 1], m = kl < pl ? kl : pl;
    const gptr<const uint8_t> a = to_global(keys) + key_off[i - 1], b = to_global(keys) + key_off[i];
    bool diff = false;
    while (l + 8 <= m) {
      const uint64_t x = *(gptr<const u64_a1>)(a + l) ^ *(gptr<const u64_a1>)(b + l);
      if (x) {
        l += (uint32_t)__builtin_ctzll(x) >> 3;
        diff = true;
        break;
      }
      l += 8;
    }
    if (!diff)
      while (l < m && a[l] == b[l]) ++l;
  }
  const uint32_t s = vl(l) + vl(kl - l) + vl(vlen) + (kl - l) + vlen;
  const uint32_t f = 1u + vl(kl) + vl(vlen) + kl + vlen;
  lcp[i] = l;
  sh[i] = s;
  c0[i] = (uint64_t)f - s;
  mark[i] = i == 0 ? 1u : 0u;
}

// ---- step 2: one doubling pass of the stride-R prefix -------------------

__global__ __launch_bounds__(256) void stride_pass_kernel(const uint64_t* __restrict__ in,
                                                          uint64_t* __restrict__ out,
                                                          uint32_t step, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = in[i] + (i >= step ? in[i - step] : 0);
}

// ---- step 3 ---------------------------------------------------------------

// ldb_blockgen_size_estimate after entries s..j of a block that starts at s.
__device__ __forceinline__ uint64_t estimate(const uint64_t* __restrict__ S,
                                             const uint64_t* __restrict__ C, uint32_t R,
                                             uint32_t s, uint32_t j) {
  const uint32_t q = (j - s) / R;
  return S[j + 1] - S[s] + C[s + q * R] - (s >= R ? C[s - R] : 0) + 4ull * (q + 1) + 4;
}

// The first index in (s, e) whose forced flag is set, e when there is none:
// F is the flags' exclusive scan (F[i] = the flags before i, F[n] their sum),
// so the flags in [s + 1, j] number F[j + 1] - F[s + 1].  s < e <= n.
__device__ __forceinline__ uint32_t first_forced(const uint64_t* __restrict__ F, uint32_t s,
                                                 uint32_t e) {
  const uint64_t base = F[s + 1];
  if (F[e] == base) return e;
  uint32_t lo = s + 1, hi = e - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (F[mid + 1] > base) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

template <bool kForced>
__global__ __launch_bounds__(256) void next_kernel(const uint64_t* __restrict__ S,
                                                   const uint64_t* __restrict__ C,
                                                   uint64_t block_size, uint32_t R,
                                                   const uint64_t* __restrict__ F,
                                                   uint32_t* __restrict__ next, uint32_t n) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  // The first j >= s whose estimate reaches block_size (table_builder.c:251-
  // 254), by doubling steps from s, then bisection; n when there is none.
  uint32_t lo = s, hi = n, probe = s, step = 1;
  for (;;) {
    if (estimate(S, C, R, s, probe) >= block_size) {
      hi = probe;
      break;
    }
    lo = probe + 1;
    if (lo >= n) break;
    probe = n - 1 - probe > step ? probe + step : n - 1;
    if (step < (1u << 30)) step <<= 1;
  }
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (estimate(S, C, R, s, mid) >= block_size) hi = mid;
    else lo = mid + 1;
  }
  const uint32_t e = lo < n ? lo + 1 : n;
  next[s] = kForced ? first_forced(F, s, e) : e;
}

// ---- step 4: one round of pointer doubling --------------------------------
// Marks written in this round may be seen by it: they are block starts too.

__global__ __launch_bounds__(256) void jump_kernel(uint32_t* mark, const uint32_t* __restrict__ jin,
                                                   uint32_t* __restrict__ jout, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = jin[i];
  if (j < n && mark[i]) mark[j] = 1u;
  jout[i] = j < n ? jin[j] : n;
}

// Per block (the marked entries): its first entry, its length, and its index
// key's length and cut point.
__global__ __launch_bounds__(256) void blocks_kernel(
    const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
    const uint32_t* __restrict__ key_len, const uint32_t* __restrict__ lcp,
    const uint64_t* __restrict__ S, const uint64_t* __restrict__ C, uint32_t R, uint32_t trim,
    const uint32_t* __restrict__ mark, const uint64_t* __restrict__ bid,
    const uint32_t* __restrict__ next, uint32_t* __restrict__ block_first,
    uint32_t* __restrict__ raw_len, uint32_t* __restrict__ ilen, uint32_t* __restrict__ icut,
    uint64_t* __restrict__ counts, uint32_t n) {
  // The longest block: one global atomic per workgroup, not per block.
  __shared__ unsigned long long s_max;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    if (!mark[i]) continue;
    const uint32_t b = (uint32_t)bid[i], e = next[i];
    block_first[b] = i;
    if (e == n) block_first[b + 1] = n;
    const uint64_t len = estimate(S, C, R, i, e - 1);   // the finished size
    raw_len[b] = (uint32_t)len;
    atomicMax(&s_max, (unsigned long long)len);
    // comparator.c:44-88 on the last key (dbformat.c:232-285: on its user key,
    // kept only when that gets shorter).
    const uint32_t la = e - 1, kla = key_len[la], ua = kla - trim;
    const gptr<const uint8_t> a = to_global(keys) + key_off[la];
    uint32_t cut = kNoCut;
    if (e < n) {
      const uint32_t ub = key_len[e] - trim, m = ua < ub ? ua : ub;
      const uint32_t d = lcp[e] < m ? lcp[e] : m;
      if (d < m) {
        const uint32_t x = a[d], y = (to_global(keys) + key_off[e])[d];
        if (x < 0xffu && x + 1 < y) cut = d;
      }
    } else {
      for (uint32_t t = 0; t < ua; ++t)
        if (a[t] != 0xffu) {
          cut = t;
          break;
        }
    }
    if (trim && cut != kNoCut && cut + 1 >= ua) cut = kNoCut;   // not physically shorter
    icut[b] = cut;
    ilen[b] = cut == kNoCut ? kla : cut + 1 + trim;
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_max) atomicMax((unsigned long long*)&counts[2], s_max);
}

__global__ void totals_kernel(uint64_t* __restrict__ raw_off, uint64_t* __restrict__ ikey_off,
                              const uint64_t* __restrict__ counts, uint32_t n) {
  raw_off[n] = counts[1];
  ikey_off[n] = counts[3];
}

// ---- step 5 ---------------------------------------------------------------

// len bytes from s to d by the G lanes of a group (lane gl): whole 16-byte
// destination granules with one unaligned load and one aligned store, the
// ragged ends byte by byte (pack_kernel's copy, lgs_table.hip).  Reads and
// writes stay inside [s, s + len) and [d, d + len).
__device__ __forceinline__ void copy_span(gptr<const uint8_t> s, gptr<uint8_t> d, uint32_t len,
                                          uint32_t gl) {
  if (len == 0) return;
  const uint64_t d0 = (uint64_t)(uintptr_t)d;
  const uint64_t g_lo = d0 & ~15ull, g_hi = (d0 + len + 15) & ~15ull;
  for (uint64_t g = g_lo + 16ull * gl; g < g_hi; g += 16ull * kGroup) {
    const int64_t k0 = (int64_t)(g - d0);
    if (g >= d0 && g + 16 <= d0 + len) {
      *(gptr<u32x4>)(d + k0) = *(gptr<const u32x4_a1>)(s + k0);
    } else {
      for (uint32_t t = 0; t < 16; ++t) {
        const int64_t k = k0 + t;
        if (k >= 0 && k < (int64_t)len) d[k] = s[k];
      }
    }
  }
}

__global__ __launch_bounds__(256) void emit_kernel(
    const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
    const uint32_t* __restrict__ key_len, const uint8_t* __restrict__ vals,
    const uint64_t* __restrict__ val_off, const uint32_t* __restrict__ val_len,
    const uint32_t* __restrict__ lcp, const uint64_t* __restrict__ S,
    const uint64_t* __restrict__ C, uint32_t R, const uint32_t* __restrict__ mark,
    const uint64_t* __restrict__ bid, const uint32_t* __restrict__ block_first,
    const uint64_t* __restrict__ raw_off, const uint32_t* __restrict__ raw_len,
    uint8_t* __restrict__ raw, uint32_t n) {
  const uint32_t gl = threadIdx.x & (kGroup - 1);
  const uint32_t groups = gridDim.x * (256 / kGroup);
  for (uint32_t i = blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup; i < n; i += groups) {
    const uint32_t b = (uint32_t)bid[i] - (mark[i] ? 0u : 1u);
    const uint32_t s = block_first[b], k = i - s;
    const gptr<uint8_t> blk = to_global(raw) + raw_off[b];
    uint32_t at = 0;
    if (k > 0)
      at = (uint32_t)(S[i] - S[s] + C[s + (k - 1) / R * R] - (s >= R ? C[s - R] : 0));
    const bool restart = k % R == 0;                 // block_builder.c:105-115
    const uint32_t shared = restart ? 0u : lcp[i];
    const uint32_t kl = key_len[i], ns = kl - shared, vlen = val_len[i];
    if (gl == 0) {                                   // :123-125
      uint32_t p = put_varint32(blk, at, shared);
      p = put_varint32(blk, p, ns);
      put_varint32(blk, p, vlen);
    }
    const uint32_t body = at + vl(shared) + vl(ns) + vl(vlen);
    copy_span(to_global(keys) + key_off[i] + shared, blk + body, ns, gl);       // :128
    copy_span(to_global(vals) + val_off[i], blk + body + ns, vlen, gl);         // :129
    if (restart && gl < 4) {                         // :143-146
      const uint32_t len = raw_len[b], m = block_first[b + 1] - s, nr = (m + R - 1) / R;
      blk[len - 4 - 4 * nr + 4 * (k / R) + gl] = (uint8_t)(at >> (8 * gl));
      if (k == 0) blk[len - 4 + gl] = (uint8_t)(nr >> (8 * gl));
    }
  }
}

__global__ __launch_bounds__(256) void ikey_kernel(
    const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
    const uint32_t* __restrict__ key_len, const uint32_t* __restrict__ block_first,
    const uint32_t* __restrict__ icut, const uint64_t* __restrict__ ikey_off,
    uint8_t* __restrict__ ikey, uint32_t trim, uint32_t nblocks) {
  const uint32_t gl = threadIdx.x & (kGroup - 1);
  const uint32_t b = blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup;
  if (b >= nblocks) return;
  const uint32_t la = block_first[b + 1] - 1, cut = icut[b];
  const gptr<const uint8_t> a = to_global(keys) + key_off[la];
  const gptr<uint8_t> d = to_global(ikey) + ikey_off[b];
  if (cut == kNoCut) {
    copy_span(a, d, key_len[la], gl);
    return;
  }
  copy_span(a, d, cut, gl);
  if (gl == 0) d[cut] = (uint8_t)(a[cut] + 1u);      // comparator.c:65, :81
  // pack_seqtype(LDB_MAX_SEQUENCE, LDB_VALTYPE_SEEK) as a fixed64 (dbformat.c:251).
  if (trim && gl < 8) d[cut + 1 + gl] = gl == 0 ? (uint8_t)0x01 : (uint8_t)0xff;
}

__global__ __launch_bounds__(256) void handle_values_kernel(
    const uint64_t* __restrict__ hoff, const uint64_t* __restrict__ hsize,
    const uint64_t* __restrict__ fstart, const uint64_t* __restrict__ ikey_off, uint32_t nblocks,
    uint8_t* __restrict__ val, uint64_t* __restrict__ val_off, uint32_t* __restrict__ val_len,
    uint32_t* __restrict__ key_len) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nblocks) return;
  const gptr<uint8_t> p = to_global(val) + 20ull * b;
  const uint64_t off = hoff[b] - (fstart ? fstart[b] : 0);   // from its file's start
  uint32_t at = 0;
  for (uint32_t w = 0; w < 2; ++w) {                 // ldb_varint64_write twice, format.c:51-52
    uint64_t v = w ? hsize[b] : off;
    while (v >= 128) {
      p[at++] = (uint8_t)(v | 128);
      v >>= 7;
    }
    p[at++] = (uint8_t)v;
  }
  val_off[b] = 20ull * b;
  val_len[b] = at;
  key_len[b] = (uint32_t)(ikey_off[b + 1] - ikey_off[b]);
}

__global__ void pair_lens_kernel(const uint32_t* __restrict__ first,
                                 const uint64_t* __restrict__ total, uint32_t* __restrict__ out) {
  out[0] = first[0];
  out[1] = (uint32_t)*total;
}

// ---- output files --------------------------------------------
// ldb_tablegen_size moves only with a block flush and compaction compares it
// after every add (db_impl.c:1417-1425), so a file ends after the first block
// whose framed end is max_size or more past the file's start: the cut's steps
// 3 and 4 once more, over blocks.

__device__ __forceinline__ uint64_t framed_end(const uint64_t* __restrict__ hoff,
                                               const uint64_t* __restrict__ hsize, uint32_t b) {
  return hoff[b] + hsize[b] + 5;                     // contents, type, crc (table_builder.c:150)
}

// Per block: the forced flag of its first entry.
__global__ __launch_bounds__(256) void block_flags_kernel(const uint32_t* __restrict__ forced,
                                                          const uint32_t* __restrict__ block_first,
                                                          uint32_t* __restrict__ fflag,
                                                          uint32_t nb) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b < nb) fflag[b] = forced[block_first[b]] ? 1u : 0u;
}

template <bool kForced>
__global__ __launch_bounds__(256) void file_next_kernel(const uint64_t* __restrict__ hoff,
                                                        const uint64_t* __restrict__ hsize,
                                                        uint64_t max_size,
                                                        const uint64_t* __restrict__ F,
                                                        uint32_t* __restrict__ next,
                                                        uint32_t* __restrict__ mark, uint32_t nb) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nb) return;
  const uint64_t start = hoff[s];
  uint32_t lo = s, hi = nb, probe = s, step = 1;
  for (;;) {
    if (framed_end(hoff, hsize, probe) - start >= max_size) {
      hi = probe;
      break;
    }
    lo = probe + 1;
    if (lo >= nb) break;
    probe = nb - 1 - probe > step ? probe + step : nb - 1;
    if (step < (1u << 30)) step <<= 1;
  }
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (framed_end(hoff, hsize, mid) - start >= max_size) hi = mid;
    else lo = mid + 1;
  }
  const uint32_t e = lo < nb ? lo + 1 : nb;
  next[s] = kForced ? first_forced(F, s, e) : e;
  mark[s] = s == 0 ? 1u : 0u;
}

// The index key of a file's last block is the short successor of its last
// key (table_builder.c:332-341), not the separator blocks_kernel chose.
__global__ __launch_bounds__(256) void file_last_keys_kernel(
    const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
    const uint32_t* __restrict__ key_len, const uint32_t* __restrict__ block_first,
    const uint32_t* __restrict__ fmark, uint32_t trim, uint32_t* __restrict__ ilen,
    uint32_t* __restrict__ icut, uint32_t nb) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb || (b + 1 < nb && !fmark[b + 1])) return;
  const uint32_t la = block_first[b + 1] - 1, kla = key_len[la], ua = kla - trim;
  const gptr<const uint8_t> a = to_global(keys) + key_off[la];
  uint32_t cut = kNoCut;
  for (uint32_t t = 0; t < ua; ++t)                  // comparator.c:72-88
    if (a[t] != 0xffu) {
      cut = t;
      break;
    }
  if (trim && cut != kNoCut && cut + 1 >= ua) cut = kNoCut;   // dbformat.c:267-285
  icut[b] = cut;
  ilen[b] = cut == kNoCut ? kla : cut + 1 + trim;
}

// Per file f (the marked blocks): its first block, first entry, start in the
// framed stream and first index-key byte; entry [files] of each is the end.
__global__ __launch_bounds__(256) void file_rows_kernel(
    const uint32_t* __restrict__ fmark, const uint64_t* __restrict__ fid,
    const uint32_t* __restrict__ fnext, const uint32_t* __restrict__ block_first,
    const uint64_t* __restrict__ hoff, const uint64_t* __restrict__ hsize,
    const uint64_t* __restrict__ ikey_off, uint32_t* __restrict__ file_block,
    uint32_t* __restrict__ file_entry, uint64_t* __restrict__ file_start,
    uint64_t* __restrict__ file_ikey, uint32_t nb) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb || !fmark[b]) return;
  const uint32_t f = (uint32_t)fid[b];
  file_block[f] = b;
  file_entry[f] = block_first[b];
  file_start[f] = hoff[b];
  file_ikey[f] = ikey_off[b];
  if (fnext[b] == nb) {
    file_block[f + 1] = nb;
    file_entry[f + 1] = block_first[nb];
    file_start[f + 1] = framed_end(hoff, hsize, nb - 1);
    file_ikey[f + 1] = ikey_off[nb];
  }
}

// Per block: its file, that file's start, its offset from there, and its
// framed length.
__global__ __launch_bounds__(256) void file_blocks_kernel(
    const uint32_t* __restrict__ fmark, const uint64_t* __restrict__ fid,
    const uint64_t* __restrict__ file_start, const uint64_t* __restrict__ hoff,
    const uint64_t* __restrict__ hsize, uint32_t* __restrict__ fof,
    uint64_t* __restrict__ fstart, uint64_t* __restrict__ rel, uint32_t* __restrict__ flen,
    uint32_t nb) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  const uint32_t f = (uint32_t)fid[b] - (fmark[b] ? 0u : 1u);
  fof[b] = f;
  fstart[b] = file_start[f];
  rel[b] = hoff[b] - file_start[f];
  flen[b] = (uint32_t)hsize[b] + 5u;
}

// Where block b's framed bytes go: its place in its file, at that file's image.
__global__ __launch_bounds__(256) void file_place_kernel(
    const uint32_t* __restrict__ fof, const uint64_t* __restrict__ rel,
    const uint64_t* __restrict__ file_off, uint64_t* __restrict__ dst_off, uint32_t nb) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  dst_off[b] = file_off[fof[b]] + rel[b];
}

// The footer (format.c:92-106) behind the index block, and the file's size.
__global__ void footer_kernel(const uint64_t* __restrict__ hoff,
                              const uint64_t* __restrict__ hsize,
                              const uint64_t* __restrict__ end, uint8_t* __restrict__ image,
                              uint64_t* __restrict__ file_size) {
  const gptr<uint8_t> p = to_global(image) + *end;
  uint32_t at = 0;
  for (uint32_t w = 0; w < 4; ++w) {                 // metaindex handle, index handle
    uint64_t v = w & 1 ? hsize[w >> 1] : hoff[w >> 1];
    while (v >= 128) {
      p[at++] = (uint8_t)(v | 128);
      v >>= 7;
    }
    p[at++] = (uint8_t)v;
  }
  while (at < 40) p[at++] = 0;
  const uint64_t magic = 0xdb4775248b80fb57ull;      // LDB_TABLE_MAGIC (format.h:26)
  for (uint32_t i = 0; i < 8; ++i) p[40 + i] = (uint8_t)(magic >> (8 * i));
  *file_size = *end + 48;
}

uint32_t grid256(uint32_t n) { return (n + 255) / 256; }

}  // namespace

int block_c_final(uint32_t n, uint32_t R) {
  int passes = 0;
  for (uint64_t step = R; step < n; step <<= 1) ++passes;
  return passes & 1;
}

hipError_t launch_block_cut(const BlockIn& in, uint64_t block_size, uint32_t R, uint32_t trim,
                            const uint32_t* forced, const BlockScratch& w, const BlockCut& out,
                            hipStream_t s) {
  const uint32_t n = in.n;
  hipError_t e = hipMemsetAsync(out.counts, 0, 8 * kBlockCounts, s);
  if (e != hipSuccess) return e;
  if (n == 0) return hipMemsetAsync(out.block_first, 0, 4, s);
  if ((e = hipMemsetAsync(out.raw_len, 0, 4 * (size_t)n, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.ilen, 0, 4 * (size_t)n, s)) != hipSuccess) return e;
  const dim3 g(grid256(n)), t(256);
  hipLaunchKernelGGL(sizes_kernel, g, t, 0, s, in.keys, in.key_off, in.key_len, in.val_len, w.lcp,
                     w.sh, w.ca, w.mark, n);
  if ((e = launch_scan(2, nullptr, w.sh, w.part, 0, w.S, w.S + n, n, s)) != hipSuccess) return e;
  uint64_t* c = w.ca;
  uint64_t* c2 = w.cb;
  for (uint64_t step = R; step < n; step <<= 1) {
    hipLaunchKernelGGL(stride_pass_kernel, g, t, 0, s, c, c2, (uint32_t)step, n);
    uint64_t* x = c;
    c = c2;
    c2 = x;
  }
  if (forced) {
    if ((e = launch_scan(2, nullptr, forced, w.part, 0, w.fs, w.fs + n, n, s)) != hipSuccess)
      return e;
    hipLaunchKernelGGL(next_kernel<true>, g, t, 0, s, w.S, c, block_size, R, w.fs, w.next, n);
  } else {
    hipLaunchKernelGGL(next_kernel<false>, g, t, 0, s, w.S, c, block_size, R, nullptr, w.next, n);
  }
  // ceil(log2(n)) rounds reach the n-th block of a chain of single entries.
  const uint32_t* jin = w.next;
  uint32_t* jout = w.ja;
  for (uint64_t reach = 1; reach < n; reach <<= 1) {
    hipLaunchKernelGGL(jump_kernel, g, t, 0, s, w.mark, jin, jout, n);
    jin = jout;
    jout = jout == w.ja ? w.jb : w.ja;
  }
  if ((e = launch_scan(2, nullptr, w.mark, w.part, 0, w.bid, out.counts, n, s)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(blocks_kernel, dim3(g.x < 2048u ? g.x : 2048u), t, 0, s, in.keys, in.key_off,
                     in.key_len, w.lcp, w.S, c, R, trim, w.mark, w.bid, w.next, out.block_first,
                     out.raw_len, w.ilen, w.icut, out.counts, n);
  if ((e = launch_scan(2, nullptr, out.raw_len, w.part, 0, out.raw_off, out.counts + 1, n, s)) !=
      hipSuccess)
    return e;
  if ((e = launch_scan(2, nullptr, w.ilen, w.part, 0, out.ikey_off, out.counts + 3, n, s)) !=
      hipSuccess)
    return e;
  hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(1), 0, s, out.raw_off, out.ikey_off, out.counts,
                     n);
  return hipGetLastError();
}

hipError_t launch_block_emit(const BlockIn& in, uint32_t R, uint32_t trim, uint32_t nblocks,
                             const BlockScratch& w, const uint32_t* block_first,
                             const uint64_t* raw_off, const uint32_t* raw_len, uint8_t* raw,
                             const uint64_t* ikey_off, uint8_t* ikey, hipStream_t s) {
  if (in.n == 0 || nblocks == 0) return hipSuccess;
  const uint64_t* c = block_c_final(in.n, R) ? w.cb : w.ca;
  const uint32_t per = 256 / kGroup;
  const uint32_t want = (in.n + per - 1) / per;
  hipLaunchKernelGGL(emit_kernel, dim3(want < 65536u ? want : 65536u), dim3(256), 0, s, in.keys,
                     in.key_off, in.key_len, in.vals, in.val_off, in.val_len, w.lcp, w.S, c, R,
                     w.mark, w.bid, block_first, raw_off, raw_len, raw, in.n);
  if (ikey)
    hipLaunchKernelGGL(ikey_kernel, dim3((nblocks + per - 1) / per), dim3(256), 0, s, in.keys,
                       in.key_off, in.key_len, block_first, w.icut, ikey_off, ikey, trim, nblocks);
  return hipGetLastError();
}

hipError_t launch_block_ikeys(const BlockIn& in, uint32_t trim, uint32_t nblocks,
                              const BlockScratch& w, const uint32_t* block_first,
                              const uint64_t* ikey_off, uint8_t* ikey, hipStream_t s) {
  if (in.n == 0 || nblocks == 0) return hipSuccess;
  const uint32_t per = 256 / kGroup;
  hipLaunchKernelGGL(ikey_kernel, dim3((nblocks + per - 1) / per), dim3(256), 0, s, in.keys,
                     in.key_off, in.key_len, block_first, w.icut, ikey_off, ikey, trim, nblocks);
  return hipGetLastError();
}

hipError_t launch_handle_values(const uint64_t* hoff, const uint64_t* hsize,
                                const uint64_t* fstart, const uint64_t* ikey_off,
                                uint32_t nblocks, uint8_t* val, uint64_t* val_off,
                                uint32_t* val_len, uint32_t* key_len, hipStream_t s) {
  if (nblocks == 0) return hipSuccess;
  hipLaunchKernelGGL(handle_values_kernel, dim3(grid256(nblocks)), dim3(256), 0, s, hoff, hsize,
                     fstart, ikey_off, nblocks, val, val_off, val_len, key_len);
  return hipGetLastError();
}

hipError_t launch_file_plan(const BlockIn& in, uint32_t trim, uint32_t nb, const uint64_t* hoff,
                            const uint64_t* hsize, uint64_t max_size, const uint32_t* forced,
                            const BlockScratch& w, const BlockCut& cut, const FilePlan& p,
                            hipStream_t s) {
  if (nb == 0) return hipSuccess;
  const dim3 g(grid256(nb)), t(256);
  if (forced) {
    hipLaunchKernelGGL(block_flags_kernel, g, t, 0, s, forced, cut.block_first, p.fflag, nb);
    const hipError_t fe = launch_scan(2, nullptr, p.fflag, w.part, 0, p.ffs, p.ffs + nb, nb, s);
    if (fe != hipSuccess) return fe;
    hipLaunchKernelGGL(file_next_kernel<true>, g, t, 0, s, hoff, hsize, max_size, p.ffs, p.next,
                       p.mark, nb);
  } else {
    hipLaunchKernelGGL(file_next_kernel<false>, g, t, 0, s, hoff, hsize, max_size, nullptr, p.next,
                       p.mark, nb);
  }
  // ceil(log2(nb)) rounds reach the nb-th file of a chain of single blocks.
  const uint32_t* jin = p.next;
  uint32_t* jout = p.ja;
  for (uint64_t reach = 1; reach < nb; reach <<= 1) {
    hipLaunchKernelGGL(jump_kernel, g, t, 0, s, p.mark, jin, jout, nb);
    jin = jout;
    jout = jout == p.ja ? p.jb : p.ja;
  }
  hipError_t e = launch_scan(2, nullptr, p.mark, w.part, 0, p.fid, p.count, nb, s);
  if (e != hipSuccess) return e;
  // The index keys of the files' last blocks, then every key's place again.
  hipLaunchKernelGGL(file_last_keys_kernel, g, t, 0, s, in.keys, in.key_off, in.key_len,
                     cut.block_first, p.mark, trim, w.ilen, w.icut, nb);
  if ((e = launch_scan(2, nullptr, w.ilen, w.part, 0, cut.ikey_off, cut.counts + 3, in.n, s)) !=
      hipSuccess)
    return e;
  hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(1), 0, s, cut.raw_off, cut.ikey_off, cut.counts,
                     in.n);
  hipLaunchKernelGGL(file_rows_kernel, g, t, 0, s, p.mark, p.fid, p.next, cut.block_first, hoff,
                     hsize, cut.ikey_off, p.file_block, p.file_entry, p.file_start, p.file_ikey,
                     nb);
  hipLaunchKernelGGL(file_blocks_kernel, g, t, 0, s, p.mark, p.fid, p.file_start, hoff, hsize,
                     p.fof, p.fstart, p.rel, p.flen, nb);
  return hipGetLastError();
}

hipError_t launch_file_place(const FilePlan& p, const uint64_t* file_off, uint64_t* dst_off,
                             uint32_t nb, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(file_place_kernel, dim3(grid256(nb)), dim3(256), 0, s, p.fof, p.rel, file_off,
                     dst_off, nb);
  return hipGetLastError();
}

hipError_t launch_footer(const uint64_t* hoff, const uint64_t* hsize, const uint64_t* end,
                         uint8_t* image, uint64_t* file_size, hipStream_t s) {
  hipLaunchKernelGGL(footer_kernel, dim3(1), dim3(1), 0, s, hoff, hsize, end, image, file_size);
  return hipGetLastError();
}

hipError_t launch_pair_lens(const uint32_t* first, const uint64_t* total, uint32_t* out,
                            hipStream_t s) {
  hipLaunchKernelGGL(pair_lens_kernel, dim3(1), dim3(1), 0, s, first, total, out);
  return hipGetLastError();
}

}  // namespace lgs
