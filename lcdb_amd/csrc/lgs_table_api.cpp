// lgs_table_api.cpp -- the SSTable runtime of the C ABI: block framing, the
// filter block, the data-block builder and whole tables, point lookups,
// opened tables and forward scans (declarations: include/lcdb_gpu_snappy.h).
// The runtime core it stands on (contexts, leases, staging, errors) is
// lgs_api.cpp's, through lgs_host.h.

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "lgs_host.h"

#include "lgs_block.h"
#include "lgs_scan.h"
#include "lgs_seek.h"
#include "lgs_table_tail.h"

namespace lgs {

// off[i] = i * stride (lgs_table.hip; declared here, not in lgs_launch.h,
// whose text keys the codec kernels' traffic figures).
hipError_t launch_fill_stride(uint64_t* off, uint64_t stride, uint32_t n, hipStream_t s);
// check_kernel's checks with one lane per handle, no CRC (lgs_table.hip;
// declared here for the same reason).
hipError_t launch_check_lane(const CheckArgs& a, hipStream_t s);

}  // namespace lgs

using namespace lgs;

extern "C" {

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
  stage_keys(keys, key_off, key_len, nq, h + o_k, (uint64_t*)(h + o_koff), (uint32_t*)(h + o_klen));
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
  size_t lcp, sh, S, ca, cb, next, ja, jb, mark, bid, icut, ilen, part, fs, total;
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
    fs = L.take(8 * m);
    total = L.at;
  }
  BlockScratch at(uint8_t* p) const {
    return BlockScratch{(uint32_t*)(p + lcp), (uint32_t*)(p + sh), (uint64_t*)(p + S),
                        (uint64_t*)(p + ca), (uint64_t*)(p + cb), (uint32_t*)(p + next),
                        (uint32_t*)(p + ja), (uint32_t*)(p + jb), (uint32_t*)(p + mark),
                        (uint64_t*)(p + bid), (uint32_t*)(p + icut), (uint32_t*)(p + ilen),
                        (uint64_t*)(p + part), (uint64_t*)(p + fs)};
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
  return lgs_block_cut_forced_dev(d_keys, d_key_off, d_key_len, d_val_len, n, block_size,
                                  restart_interval, internal_keys, nullptr, d_block_first,
                                  d_raw_off, d_raw_len, d_ikey_off, d_counts, d_scratch,
                                  scratch_bytes, stream);
}

int lgs_block_cut_forced_dev(const uint8_t* d_keys, const uint64_t* d_key_off,
                             const uint32_t* d_key_len, const uint32_t* d_val_len, uint32_t n,
                             uint64_t block_size, uint32_t restart_interval, int internal_keys,
                             const uint32_t* d_forced, uint32_t* d_block_first,
                             uint64_t* d_raw_off, uint32_t* d_raw_len, uint64_t* d_ikey_off,
                             uint64_t* d_counts, void* d_scratch, size_t scratch_bytes,
                             void* stream) {
  LGS_TRY(block_args(n, restart_interval, internal_keys));
  if (!d_block_first || !d_raw_off || !d_raw_len || !d_ikey_off || !d_counts || !d_scratch ||
      (n && (!d_keys || !d_key_off || !d_key_len || !d_val_len)))
    return fail(LGS_EINVAL, "NULL argument");
  const BlockBuildScratch B(n);
  if (scratch_bytes < B.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_block_build_scratch)", scratch_bytes, B.total);
  const BlockIn in{d_keys, d_key_off, d_key_len, nullptr, nullptr, d_val_len, n};
  const BlockCut out{d_block_first, d_raw_off, d_raw_len, d_ikey_off, d_counts};
  LGS_HIP(launch_block_cut(in, block_size, restart_interval, internal_keys ? 8u : 0u, d_forced,
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
  LGS_HIP(launch_block_cut(in, block_size, restart_interval, trim, nullptr, B.at(d + o_scr), cut,
                           c.stream));
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

// ---- whole tables: lgs_table_build_host and lgs_tables_build_dev ----
//
// Both are a data stage (cut, emit, frame: one framed stream of data blocks
// with their handles) and a tail stage per file (index block, filter block,
// metaindex, footer); the host call uploads before and downloads after, the
// device call plans compaction's output files in between.

namespace {

// A table build's part of the arena: the tail's uploads and the small
// downloads (pinned on the host side), then what lives on the device only.
struct BuildLayout {
  uint32_t n = 0, icap = 0;
  bool filter = false;
  size_t raw_bound = 0, fbound = 0, ibound = 0, wtotal = 0, bscr = 0, fscr = 0;
  uint64_t data_bound = 0;
  size_t o_ftoff = 0, o_ftlen = 0;                                     // the filter block's {offset, length}
  size_t o_meta = 0, o_toff = 0, o_tlen = 0, o_tencoff = 0, o_titems = 0;   // one upload
  size_t o_cnt = 0, o_cnt2 = 0, o_end = 0, o_fsize = 0, o_size = 0, o_nfiles = 0, pin_end = 0;
  CutLayout K, K2;
  size_t o_raw = 0, o_ikey = 0, o_scr = 0, o_wscr = 0, o_hoff = 0, o_hsize = 0, o_fscr = 0,
         o_fout = 0, o_hval = 0, o_ivoff = 0, o_ivlen = 0, o_iklen = 0, o_iraw = 0, o_stream = 0,
         o_thoff = 0, o_thsize = 0, o_tslots = 0, o_tpacked = 0, o_tenclen = 0, o_tenclen2 = 0,
         o_tpoff = 0, o_tptotal = 0, o_tfoff = 0, o_tpart = 0;
  // The file plan (lgs_tables_build_dev only).
  size_t p_next = 0, p_ja = 0, p_jb = 0, p_mark = 0, p_fid = 0, p_fof = 0, p_fstart = 0,
         p_rel = 0, p_flen = 0, p_fblock = 0, p_fentry = 0, p_fbegin = 0, p_fikey = 0, p_dst = 0,
         p_fflag = 0, p_ffs = 0;

  // image: the framed stream is followed by one table's tail (the host call);
  // plan: room for the file plan.
  int take(Layout& L, uint32_t n_, uint64_t kb, uint64_t vb, int bits_per_key, bool image,
           bool plan) {
    n = n_;
    filter = bits_per_key > 0;
    raw_bound = lgs_block_build_bound(n, kb, vb);
    data_bound = raw_bound + (uint64_t)LGS_TRAILER_SIZE * n;
    if (data_bound >= kMaxDataEnd) return fail(LGS_EINVAL, "table of %llu bytes too large",
                                               (unsigned long long)data_bound);
    fbound = filter ? lgs_filter_block_bound(n, n, data_bound, bits_per_key) : 0;
    ibound = index_block_bound(n, kb);
    if (fbound > 0x7fffffffull || ibound > 0x7fffffffull)
      return fail(LGS_EINVAL, "filter or index block over 2^31 bytes");
    bscr = BlockBuildScratch(n).total;
    fscr = FilterScratch(data_bound).total;
    wtotal = WriteScratch(n, raw_bound).total;
    if (WriteScratch(1, fbound).total > wtotal) wtotal = WriteScratch(1, fbound).total;
    o_ftoff = L.take(8);
    o_ftlen = L.take(8);
    o_meta = L.take(kMetaindexMax + 16);   // tail uploads: metaindex, {offset, length} x 2
    o_toff = L.take(16);
    o_tlen = L.take(8);
    o_tencoff = L.take(16);
    // The tail's encoder items: the metaindex block and the index block's 64 KiB
    // chunks ({input offset, output slot} u64, {length, header} u32 each).
    icap = 2 + (uint32_t)(ibound / kChunk);
    o_titems = L.take(24 * (size_t)icap);
    o_cnt = L.take(8 * kBlockCounts);      // downloads
    o_cnt2 = L.take(8 * kBlockCounts);
    o_end = L.take(8);
    o_fsize = L.take(8);
    o_size = L.take(8);
    o_nfiles = L.take(8);
    pin_end = L.at;
    K.take(L, n);
    K2.take(L, n);
    o_raw = L.take(raw_bound);
    o_ikey = L.take((size_t)kb + 16);
    o_scr = L.take(bscr);
    o_wscr = L.take(wtotal);
    o_hoff = L.take(8 * (size_t)n + 8);
    o_hsize = L.take(8 * (size_t)n + 8);
    o_fscr = L.take(fscr);
    o_fout = L.take(fbound + 16);
    o_hval = L.take(20 * (size_t)n + 16);
    o_ivoff = L.take(8 * (size_t)n + 8);
    o_ivlen = L.take(4 * (size_t)n + 4);
    o_iklen = L.take(4 * (size_t)n + 4);
    o_iraw = L.take(ibound + 16);
    o_stream = L.take((image ? lgs_table_build_bound(n, kb, vb, bits_per_key)
                             : (size_t)data_bound) + 16);
    o_thoff = L.take(16);
    o_thsize = L.take(16);
    o_tslots = L.take((size_t)icap * chunk_out(kChunk));
    o_tpacked = L.take(bound_of(ibound) + 64);
    o_tenclen = L.take(4 * (size_t)icap);
    o_tenclen2 = L.take(8);
    o_tpoff = L.take(8 * (size_t)icap);
    o_tptotal = L.take(8);
    o_tfoff = L.take(16);
    o_tpart = L.take(8 * scan_parts(icap) + 16);
    if (plan) {
      const size_t m = (size_t)n + 2;
      p_next = L.take(4 * m);
      p_ja = L.take(4 * m);
      p_jb = L.take(4 * m);
      p_mark = L.take(4 * m);
      p_fid = L.take(8 * m);
      p_fof = L.take(4 * m);
      p_fstart = L.take(8 * m);
      p_rel = L.take(8 * m);
      p_flen = L.take(4 * m);
      p_fblock = L.take(4 * m);
      p_fentry = L.take(4 * m);
      p_fbegin = L.take(8 * m);
      p_fikey = L.take(8 * m);
      p_dst = L.take(8 * m);
      p_fflag = L.take(4 * m);
      p_ffs = L.take(8 * m);
    }
    return LGS_OK;
  }
  FilePlan plan_at(uint8_t* p) const {
    return FilePlan{(uint32_t*)(p + p_next), (uint32_t*)(p + p_ja), (uint32_t*)(p + p_jb),
                    (uint32_t*)(p + p_mark), (uint64_t*)(p + p_fid), (uint32_t*)(p + p_fof),
                    (uint64_t*)(p + p_fstart), (uint64_t*)(p + p_rel), (uint32_t*)(p + p_flen),
                    (uint32_t*)(p + p_fflag), (uint64_t*)(p + p_ffs),
                    (uint32_t*)(p + p_fblock), (uint32_t*)(p + p_fentry),
                    (uint64_t*)(p + p_fbegin), (uint64_t*)(p + p_fikey),
                    (uint64_t*)(p + o_nfiles)};
  }
};

struct DataBlocks {
  uint64_t nb = 0, raw_total = 0, max_raw = 0;
};

// The data stage: n > 0 entries on the device -> the blocks' cut, their raw
// bytes, and the framed stream from offset 0 at d + A.o_stream with its
// handles at d + A.o_hoff / o_hsize and its end in the word d + A.o_end
// (table_builder.c:215-278).  ikeys: emit the index keys with the blocks (one
// file: the cut's keys stand).  One synchronisation, for the block count.
static int build_data(const BuildLayout& A, uint8_t* h, uint8_t* d, hipStream_t s,
                      const BlockIn& in, uint64_t key_bytes, uint64_t block_size,
                      uint32_t restart_interval, uint32_t trim, const uint32_t* forced,
                      int compression, bool ikeys, DataBlocks* out) {
  const BlockBuildScratch B(A.n);
  const BlockCut cut = A.K.at(d, (uint64_t*)(d + A.o_cnt));
  LGS_HIP(launch_block_cut(in, block_size, restart_interval, trim, forced, B.at(d + A.o_scr), cut,
                           s));
  LGS_HIP(hipMemcpyAsync(h + A.o_cnt, d + A.o_cnt, 8 * kBlockCounts, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  const uint64_t* cnt = (const uint64_t*)(h + A.o_cnt);
  const uint64_t nb = cnt[0], raw_total = cnt[1], max_raw = cnt[2];
  if (nb == 0 || nb > A.n || raw_total + 16 > A.raw_bound || cnt[3] > key_bytes)
    return fail(LGS_EINTERNAL, "cut of %u entries: %llu blocks, %llu bytes", A.n,
                (unsigned long long)nb, (unsigned long long)raw_total);
  if (max_raw > 0x7fffffffull)
    return fail(LGS_EINVAL, "a block of %llu bytes: under 2^31 supported",
                (unsigned long long)max_raw);
  LGS_HIP(launch_block_emit(in, restart_interval, trim, (uint32_t)nb, B.at(d + A.o_scr),
                            cut.block_first, cut.raw_off, cut.raw_len, d + A.o_raw, cut.ikey_off,
                            ikeys ? d + A.o_ikey : nullptr, s));
  LGS_TRY(table_write(d + A.o_raw, cut.raw_off, cut.raw_len, (uint32_t)nb, (uint32_t)max_raw,
                      compression, 0, d + A.o_stream, (uint64_t*)(d + A.o_hoff),
                      (uint64_t*)(d + A.o_hsize), (uint64_t*)(d + A.o_end), d + A.o_wscr,
                      WriteScratch((uint32_t)nb, raw_total), s));
  out->nb = nb;
  out->raw_total = raw_total;
  out->max_raw = max_raw;
  return LGS_OK;
}

// One file of a build: data blocks [b0, b0 + nb) of the cut, whose ne entries
// start at the cut's block_first[b0]; the data region's bytes are in place at
// `image`, and the index entries (keys at d + A.o_ikey, handle values at
// d + A.o_hval) are made.
struct TailFile {
  uint32_t b0 = 0, nb = 0, ne = 0;
  // The data region's length; unknown: the word d + A.o_end holds it, and the
  // tail synchronises once more to read it.
  bool len_known = false;
  uint64_t data_len = 0;
  const uint64_t* block_off = nullptr;   // device: the nb blocks' offsets in the file
  uint8_t* image = nullptr;              // device: the file's first byte
  uint64_t* d_size = nullptr;            // device: receives the file's size
};

// The tail stage (table_builder.c:280-365): the index block of the file's
// entries, the filter block of its keys, the metaindex, both framed through
// the table's compression behind the data region, and the footer.  Counts
// come back in one synchronisation (two when the data length is not known);
// what it queues after that is complete on the stream, not on return.  The
// pinned words it uploads from are rewritten only behind the next
// synchronisation of this stream, this function's own included.
static int build_tail(const BuildLayout& A, uint8_t* h, uint8_t* d, hipStream_t s,
                      const BlockIn& in, int compression, int bits_per_key, int internal_keys,
                      const TailFile& f) {
  const BlockBuildScratch B(A.n);
  const BlockCut cut = A.K.at(d, (uint64_t*)(d + A.o_cnt));
  const BlockCut cut2 = A.K2.at(d, (uint64_t*)(d + A.o_cnt2));
  const BlockIn iin{d + A.o_ikey, cut.ikey_off + f.b0, (const uint32_t*)(d + A.o_iklen) + f.b0,
                    d + A.o_hval, (const uint64_t*)(d + A.o_ivoff) + f.b0,
                    (const uint32_t*)(d + A.o_ivlen) + f.b0, f.nb};
  uint64_t data_len = f.data_len, index_len = 0, filter_size = 0;
  const auto build_filter = [&]() -> int {       // table_builder.c:242-243, :276-277, :292-295
    LGS_TRY(lgs_filter_block_build_dev(in.keys, in.key_off, in.key_len, f.ne,
                                       cut.block_first + f.b0, f.block_off, f.nb, data_len,
                                       bits_per_key, internal_keys, d + A.o_fout, A.fbound,
                                       (uint64_t*)(d + A.o_fsize), d + A.o_fscr, A.fscr, s));
    LGS_HIP(hipMemcpyAsync(h + A.o_fsize, d + A.o_fsize, 8, hipMemcpyDeviceToHost, s));
    return LGS_OK;
  };
  if (A.filter && f.len_known) LGS_TRY(build_filter());
  if (f.nb) {
    // The index block's entries (:229-239, :332-341): index key -> handle, one
    // block whatever its size, restart interval 1 (:87).
    LGS_HIP(launch_block_cut(iin, ~0ull, 1, 0, nullptr, B.at(d + A.o_scr), cut2, s));
    LGS_HIP(hipMemcpyAsync(h + A.o_cnt2, d + A.o_cnt2, 8 * kBlockCounts, hipMemcpyDeviceToHost, s));
    if (!f.len_known)
      LGS_HIP(hipMemcpyAsync(h + A.o_end, d + A.o_end, 8, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    if (!f.len_known) data_len = *(const uint64_t*)(h + A.o_end);
    const uint64_t* cnt2 = (const uint64_t*)(h + A.o_cnt2);
    index_len = cnt2[1];
    if (data_len > A.data_bound || cnt2[0] != 1 || index_len > A.ibound)
      return fail(LGS_EINTERNAL, "data blocks end at %llu, index block of %llu bytes",
                  (unsigned long long)data_len, (unsigned long long)index_len);
    LGS_HIP(launch_block_emit(iin, 1, 0, 1, B.at(d + A.o_scr), cut2.block_first, cut2.raw_off,
                              cut2.raw_len, d + A.o_iraw, nullptr, nullptr, s));
  } else {
    // An index block with no entries (block_builder.c:68, :143-146).
    LGS_HIP(hipStreamSynchronize(s));
    index_len = tail_metaindex(h + A.o_meta, kMetaindexMax, nullptr, 0, 0);
    LGS_HIP(hipMemcpyAsync(d + A.o_iraw, h + A.o_meta, (size_t)index_len, hipMemcpyHostToDevice, s));
    LGS_HIP(hipStreamSynchronize(s));
  }
  // The filter block (:292-299), stored raw after the data blocks.
  uint64_t at = data_len;
  if (A.filter) {
    if (!f.len_known) {
      LGS_TRY(build_filter());
      LGS_HIP(hipStreamSynchronize(s));
    }
    filter_size = *(const uint64_t*)(h + A.o_fsize);
    if (filter_size > A.fbound)
      return fail(LGS_EINTERNAL, "filter block %llu > bound %zu", (unsigned long long)filter_size,
                  A.fbound);
    *(uint64_t*)(h + A.o_ftoff) = 0;
    *(uint32_t*)(h + A.o_ftlen) = (uint32_t)filter_size;
    LGS_HIP(hipMemcpyAsync(d + A.o_ftoff, h + A.o_ftoff, 8, hipMemcpyHostToDevice, s));
    LGS_HIP(hipMemcpyAsync(d + A.o_ftlen, h + A.o_ftlen, 4, hipMemcpyHostToDevice, s));
    LGS_TRY(table_write(d + A.o_fout, (const uint64_t*)(d + A.o_ftoff),
                        (const uint32_t*)(d + A.o_ftlen), 1, (uint32_t)filter_size,
                        LGS_NO_COMPRESSION, at, f.image + at, (uint64_t*)(d + A.o_thoff),
                        (uint64_t*)(d + A.o_thsize), nullptr, d + A.o_wscr,
                        WriteScratch(1, filter_size), s));
    at += filter_size + LGS_TRAILER_SIZE;
  }
  // Metaindex (:301-328) and index (:330-344) blocks, both through the
  // table's compression like every block ldb_tablegen_write_block writes.
  // The index block grows with the table (C5: 36 MB), and one block is one
  // wave's work in the encoder, 64 KiB chunk after chunk; the chunks are
  // independent (snappy.c:370-381), so they are encoded here as items of
  // their own, as ldb_snappy_encode does, and packed into the block's stream.
  const size_t meta_len = tail_metaindex(h + A.o_meta, kMetaindexMax,
                                         A.filter ? kFilterName : nullptr, data_len, filter_size);
  if (meta_len == 0) return fail(LGS_EINTERNAL, "metaindex block does not fit");
  const bool snappy = compression == LGS_SNAPPY_COMPRESSION;
  const uint32_t icap = A.icap;
  uint64_t* toff = (uint64_t*)(h + A.o_toff);
  uint32_t* tlen = (uint32_t*)(h + A.o_tlen);
  uint64_t* tenc_off = (uint64_t*)(h + A.o_tencoff);
  toff[0] = A.o_meta;          // offsets from the arena's start
  toff[1] = A.o_iraw;
  tlen[0] = (uint32_t)meta_len;
  tlen[1] = (uint32_t)index_len;
  tenc_off[0] = A.o_tslots;
  tenc_off[1] = A.o_tpacked;
  const uint32_t items = 1 + (uint32_t)((index_len + kChunk - 1) / kChunk);
  if (items > icap) return fail(LGS_EINTERNAL, "index block of %llu bytes",
                                (unsigned long long)index_len);
  uint64_t* it_in = (uint64_t*)(h + A.o_titems);
  uint64_t* it_out = it_in + icap;
  uint32_t* it_len = (uint32_t*)(it_out + icap);
  uint32_t* it_hdr = it_len + icap;
  it_in[0] = A.o_meta;
  it_len[0] = it_hdr[0] = (uint32_t)meta_len;
  it_out[0] = A.o_tslots;
  size_t slot = A.o_tslots + chunk_out((uint32_t)meta_len);
  for (uint32_t j = 1; j < items; ++j) {
    const uint64_t off = (uint64_t)(j - 1) * kChunk;
    it_in[j] = A.o_iraw + off;
    it_len[j] = (uint32_t)(index_len - off < kChunk ? index_len - off : kChunk);
    it_hdr[j] = j == 1 ? (uint32_t)index_len : 0xffffffffu;      // snappy.c:368
    it_out[j] = slot;
    slot += chunk_out(it_len[j]);
  }
  LGS_HIP(hipMemcpyAsync(d + A.o_meta, h + A.o_meta, A.o_cnt - A.o_meta, hipMemcpyHostToDevice, s));
  uint64_t* part = (uint64_t*)(d + A.o_tpart);
  uint32_t* enc_len = (uint32_t*)(d + A.o_tenclen);
  uint32_t* enc_len2 = (uint32_t*)(d + A.o_tenclen2);
  if (snappy) {
    const uint64_t* d_out = (const uint64_t*)(d + A.o_titems) + icap;
    const uint32_t* d_len = (const uint32_t*)(d_out + icap);
    EncodeArgs ea{d, (const uint64_t*)(d + A.o_titems), d_len, d, d_out, enc_len, d_len + icap,
                  nullptr, items, nullptr};
    const uint32_t ichunk = (uint32_t)(index_len < kChunk ? index_len : kChunk);
    LGS_HIP(launch_encode(ea, meta_len > ichunk ? (uint32_t)meta_len : ichunk, s));
    LGS_HIP(launch_scan(2, nullptr, enc_len + 1, part, 0, (uint64_t*)(d + A.o_tpoff),
                        (uint64_t*)(d + A.o_tptotal), items - 1, s));
    LGS_HIP(launch_pack(d, d_out + 1, enc_len + 1, d + A.o_tpacked,
                        (const uint64_t*)(d + A.o_tpoff), items - 1, s));
    LGS_HIP(launch_pair_lens(enc_len, (const uint64_t*)(d + A.o_tptotal), enc_len2, s));
  }
  LGS_HIP(launch_scan(1, (const uint32_t*)(d + A.o_tlen), snappy ? enc_len2 : nullptr, part, at,
                      (uint64_t*)(d + A.o_tfoff), (uint64_t*)(d + A.o_end), 2, s));
  const FrameArgs fa{d, (const uint64_t*)(d + A.o_toff), (const uint32_t*)(d + A.o_tlen), d,
                     (const uint64_t*)(d + A.o_tencoff), snappy ? enc_len2 : nullptr,
                     f.image + at, at, (const uint64_t*)(d + A.o_tfoff),
                     (uint64_t*)(d + A.o_thoff), (uint64_t*)(d + A.o_thsize), 2};
  LGS_HIP(launch_frame(fa, s));
  LGS_HIP(launch_footer((const uint64_t*)(d + A.o_thoff), (const uint64_t*)(d + A.o_thsize),
                        (const uint64_t*)(d + A.o_end), f.image, f.d_size, s));   // :346-362
  return LGS_OK;
}

static int build_args(uint32_t n, uint32_t restart_interval, int compression, int bits_per_key,
                      int internal_keys) {
  LGS_TRY(block_args(n, restart_interval, internal_keys));
  if (compression != LGS_NO_COMPRESSION && compression != LGS_SNAPPY_COMPRESSION)
    return fail(LGS_EINVAL, "unknown compression type %d", compression);
  if (bits_per_key < 0 || bits_per_key > kMaxBitsPerKey)
    return fail(LGS_EINVAL, "bits_per_key %d out of range", bits_per_key);
  return LGS_OK;
}

// What one output file's image may take: its data region and the bounds of
// its tail's blocks with their trailers, the footer, 16 spare bytes.
static uint64_t file_slot(uint64_t data_len, uint32_t ne, uint32_t nb, uint64_t ikey_bytes,
                          int bits_per_key) {
  const uint64_t filter =
      bits_per_key > 0 ? lgs_filter_block_bound(ne, nb, data_len, bits_per_key) + LGS_TRAILER_SIZE : 0;
  return data_len + filter + kMetaindexMax + LGS_TRAILER_SIZE + index_block_bound(nb, ikey_bytes) +
         LGS_TRAILER_SIZE + kFooterSize + 16;
}

}  // namespace

int lgs_table_build_host(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len,
                         const uint8_t* vals, const uint64_t* val_off, const uint32_t* val_len,
                         uint32_t n, uint64_t block_size, uint32_t restart_interval,
                         int compression, int bits_per_key, int internal_keys, uint8_t* file,
                         size_t file_cap, size_t* file_size) {
  LGS_TRY(build_args(n, restart_interval, compression, bits_per_key, internal_keys));
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
  const size_t img_bound = lgs_table_build_bound(n, E.kb, E.vb, bits_per_key);
  Layout L;  // uploads | small downloads | device-only
  entries_layout(L, n, &E);
  const size_t up_end = L.at;
  BuildLayout A;
  LGS_TRY(A.take(L, n, E.kb, E.vb, bits_per_key, true, false));
  LGS_TRY(ctx_reserve(c, L.at, A.pin_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  hipStream_t s = c.stream;
  const BlockIn in = entries_in(d, E, n);
  DataBlocks D;
  if (n) {
    entries_stage(h, E, keys, key_off, key_len, vals, val_off, val_len, n);
    LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, s));
    LGS_TRY(build_data(A, h, d, s, in, E.kb, block_size, restart_interval, internal_keys ? 8u : 0u,
                       nullptr, compression, true, &D));
    LGS_HIP(launch_handle_values((const uint64_t*)(d + A.o_hoff), (const uint64_t*)(d + A.o_hsize),
                                 nullptr, (const uint64_t*)(d + A.K.ioff), (uint32_t)D.nb,
                                 d + A.o_hval, (uint64_t*)(d + A.o_ivoff),
                                 (uint32_t*)(d + A.o_ivlen), (uint32_t*)(d + A.o_iklen), s));
  } else {
    LGS_HIP(hipMemsetAsync(d + A.K.bf, 0, 4, s));
  }
  TailFile f;
  f.nb = (uint32_t)D.nb;
  f.ne = n;
  f.len_known = n == 0;
  f.block_off = (const uint64_t*)(d + A.o_hoff);
  f.image = d + A.o_stream;
  f.d_size = (uint64_t*)(d + A.o_size);
  LGS_TRY(build_tail(A, h, d, s, in, compression, bits_per_key, internal_keys, f));
  LGS_HIP(hipMemcpyAsync(h + A.o_size, d + A.o_size, 8, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  const uint64_t size = *(const uint64_t*)(h + A.o_size);
  if (size > img_bound)
    return fail(LGS_EINTERNAL, "table of %llu bytes > bound %zu", (unsigned long long)size, img_bound);
  *file_size = (size_t)size;
  if (size > file_cap)
    return fail(LGS_ENOSPC, "table needs %llu bytes, file_cap %zu", (unsigned long long)size,
                file_cap);
  LGS_HIP(hipMemcpyAsync(file, d + A.o_stream, (size_t)size, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  return LGS_OK;
}

size_t lgs_tables_build_bound(uint32_t n, uint64_t key_bytes, uint64_t value_bytes,
                              int bits_per_key, uint64_t max_file_size, uint32_t* max_files) {
  return lgs_tables_build_forced_bound(n, key_bytes, value_bytes, bits_per_key, max_file_size, 0,
                                       max_files);
}

size_t lgs_tables_build_forced_bound(uint32_t n, uint64_t key_bytes, uint64_t value_bytes,
                                     int bits_per_key, uint64_t max_file_size, uint32_t n_forced,
                                     uint32_t* max_files) {
  // Every file but the last holds at least max_file_size bytes of data blocks
  // or ends before a forced start, and every file at least one entry; per
  // file the tail's constant parts, the spare bytes and the alignment of
  // file_slot (under 320 bytes).
  const uint64_t data = key_bytes + value_bytes + 19ull * n + (uint64_t)LGS_TRAILER_SIZE * n;
  uint64_t files = (max_file_size ? data / max_file_size + 1 : n) + n_forced;
  if (files > n) files = n;
  if (max_files) *max_files = (uint32_t)files;
  return (size_t)(lgs_table_build_bound(n, key_bytes, value_bytes, bits_per_key) + 320 * files);
}

int lgs_tables_build_dev(const uint8_t* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
                         const uint8_t* d_vals, const uint64_t* d_val_off, const uint32_t* d_val_len,
                         uint32_t n, uint64_t key_bytes, uint64_t value_bytes, uint64_t block_size,
                         uint32_t restart_interval, int compression, int bits_per_key,
                         int internal_keys, uint64_t max_file_size, uint8_t* d_files,
                         size_t files_cap, uint64_t* d_file_off, uint64_t* d_file_size,
                         uint32_t* d_file_first, uint32_t files_cap_count, uint32_t* n_files,
                         uint64_t* files_bytes, void* stream) {
  return lgs_tables_build_forced_dev(d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, n,
                                     key_bytes, value_bytes, block_size, restart_interval,
                                     compression, bits_per_key, internal_keys, max_file_size,
                                     nullptr, d_files, files_cap, d_file_off, d_file_size,
                                     d_file_first, files_cap_count, n_files, files_bytes, stream);
}

int lgs_tables_build_forced_dev(const uint8_t* d_keys, const uint64_t* d_key_off,
                                const uint32_t* d_key_len, const uint8_t* d_vals,
                                const uint64_t* d_val_off, const uint32_t* d_val_len, uint32_t n,
                                uint64_t key_bytes, uint64_t value_bytes, uint64_t block_size,
                                uint32_t restart_interval, int compression, int bits_per_key,
                                int internal_keys, uint64_t max_file_size,
                                const uint32_t* d_forced, uint8_t* d_files, size_t files_cap,
                                uint64_t* d_file_off, uint64_t* d_file_size,
                                uint32_t* d_file_first, uint32_t files_cap_count,
                                uint32_t* n_files, uint64_t* files_bytes, void* stream) {
  LGS_TRY(build_args(n, restart_interval, compression, bits_per_key, internal_keys));
  if (!n_files || !files_bytes) return fail(LGS_EINVAL, "NULL argument");
  *n_files = 0;
  *files_bytes = 0;
  // A file closed after every entry ends with a pending block, not after a
  // flush (db_impl.c:1417-1425 with table_builder.c:251-254).
  if (max_file_size == 0) return fail(LGS_EINVAL, "max_file_size must be at least 1");
  if (n == 0) return LGS_OK;
  if (!d_keys || !d_key_off || !d_key_len || !d_vals || !d_val_off || !d_val_len)
    return fail(LGS_EINVAL, "NULL argument");
  if (key_bytes > (1ull << 62) || value_bytes > (1ull << 62))
    return fail(LGS_EINVAL, "key_bytes or value_bytes out of range");
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  Layout L;
  BuildLayout A;
  LGS_TRY(A.take(L, n, key_bytes, value_bytes, bits_per_key, false, true));
  LGS_TRY(ctx_reserve(c, L.at, A.pin_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t trim = internal_keys ? 8u : 0u;
  const BlockIn in{d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len, n};
  DataBlocks D;
  LGS_TRY(build_data(A, h, d, s, in, key_bytes, block_size, restart_interval, trim, d_forced,
                     compression, false, &D));
  const uint32_t nb = (uint32_t)D.nb;
  // The files (second synchronisation: their number; third: one row each).
  const BlockBuildScratch B(n);
  const BlockCut cut = A.K.at(d, (uint64_t*)(d + A.o_cnt));
  const FilePlan P = A.plan_at(d);
  const uint64_t* d_hoff = (const uint64_t*)(d + A.o_hoff);
  const uint64_t* d_hsize = (const uint64_t*)(d + A.o_hsize);
  LGS_HIP(launch_file_plan(in, trim, nb, d_hoff, d_hsize, max_file_size, d_forced,
                           B.at(d + A.o_scr), cut, P, s));
  LGS_HIP(hipMemcpyAsync(h + A.o_nfiles, d + A.o_nfiles, 8, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  const uint64_t nf = *(const uint64_t*)(h + A.o_nfiles);
  if (nf == 0 || nf > nb) return fail(LGS_EINTERNAL, "%llu files of %u blocks",
                                      (unsigned long long)nf, nb);
  std::vector<uint32_t> fblock(nf + 1), fentry(nf + 1);
  std::vector<uint64_t> fbegin(nf + 1), fikey(nf + 1), foff(nf);
  LGS_HIP(hipMemcpyAsync(fblock.data(), P.file_block, 4 * (nf + 1), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(fentry.data(), P.file_entry, 4 * (nf + 1), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(fbegin.data(), P.file_start, 8 * (nf + 1), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(fikey.data(), P.file_ikey, 8 * (nf + 1), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  uint64_t total = 0;
  for (uint64_t f = 0; f < nf; ++f) {
    if (fblock[f + 1] <= fblock[f] || fentry[f + 1] <= fentry[f] || fbegin[f + 1] <= fbegin[f] ||
        fikey[f + 1] < fikey[f] || fblock[f + 1] > nb || fentry[f + 1] > n ||
        fbegin[f + 1] > A.data_bound || fikey[f + 1] > key_bytes)
      return fail(LGS_EINTERNAL, "file %llu of the plan is out of order", (unsigned long long)f);
    foff[f] = total;
    total = align_up((size_t)(total + file_slot(fbegin[f + 1] - fbegin[f], fentry[f + 1] - fentry[f],
                                                fblock[f + 1] - fblock[f],
                                                fikey[f + 1] - fikey[f], bits_per_key)), 16);
  }
  if (fblock[0] != 0 || fblock[nf] != nb || fentry[nf] != n)
    return fail(LGS_EINTERNAL, "the file plan does not cover the blocks");
  *n_files = (uint32_t)nf;
  *files_bytes = total;
  if (nf > files_cap_count || total > files_cap)
    return fail(LGS_ENOSPC, "%llu files of %llu bytes (files_cap_count %u, files_cap %zu)",
                (unsigned long long)nf, (unsigned long long)total, files_cap_count, files_cap);
  if (!d_files || !d_file_off || !d_file_size || !d_file_first)
    return fail(LGS_EINVAL, "NULL argument");
  // Everything from here is queued behind the uploads of this function's own
  // arrays and works in the pooled arena, so the stream is drained on every
  // way out.
  const int rc = [&]() -> int {
    LGS_HIP(hipMemcpyAsync(d_file_off, foff.data(), 8 * nf, hipMemcpyHostToDevice, s));
    LGS_HIP(hipMemcpyAsync(d_file_first, P.file_entry, 4 * (nf + 1), hipMemcpyDeviceToDevice, s));
    // Index keys (the files' last blocks now end in short successors), handle
    // values from each file's start, and the data regions to their images.
    LGS_HIP(launch_block_ikeys(in, trim, nb, B.at(d + A.o_scr), cut.block_first, cut.ikey_off,
                               d + A.o_ikey, s));
    LGS_HIP(launch_handle_values(d_hoff, d_hsize, P.fstart, cut.ikey_off, nb, d + A.o_hval,
                                 (uint64_t*)(d + A.o_ivoff), (uint32_t*)(d + A.o_ivlen),
                                 (uint32_t*)(d + A.o_iklen), s));
    LGS_HIP(launch_file_place(P, d_file_off, (uint64_t*)(d + A.p_dst), nb, s));
    LGS_HIP(launch_pack(d + A.o_stream, d_hoff, P.flen, d_files, (const uint64_t*)(d + A.p_dst), nb,
                        s));
    for (uint64_t f = 0; f < nf; ++f) {
      TailFile t;
      t.b0 = fblock[f];
      t.nb = fblock[f + 1] - fblock[f];
      t.ne = fentry[f + 1] - fentry[f];
      t.len_known = true;
      t.data_len = fbegin[f + 1] - fbegin[f];
      t.block_off = P.rel + t.b0;
      t.image = d_files + foff[f];
      t.d_size = d_file_size + f;
      LGS_TRY(build_tail(A, h, d, s, in, compression, bits_per_key, internal_keys, t));
    }
    return LGS_OK;
  }();
  const hipError_t drained = hipStreamSynchronize(s);
  LGS_TRY(rc);
  LGS_HIP(drained);
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

// "These n block handles, read into this arena": the one block-read stage of
// the gets, the open and the scan.  The caller lays out one arena (the pinned
// and the device one alike, see Layout) and the stage takes its fields from
// it: take_upload what the host stages, in one run behind which the caller
// may put uploads of its own, so that one hipMemcpyAsync covers both;
// take_scratch and take_output what only the device touches.  Two ways to
// fill it: a borrowed host image (plan, then stage) or a resident device image
// (plan_resident, then bind_resident).  read() is the table_read call.
struct BlockRead {
  uint32_t n = 0;
  size_t img = 0;          // a borrowed image's packed byte ranges
  size_t outb = 0;         // the blocks' 16-aligned output slots
  uint32_t max_cap = 0;
  std::vector<HandlePlan> plans;
  ReadScratch R{0};
  size_t blk = 0, hoff = 0, hsize = 0, ooff = 0, ocap = 0;   // the upload run
  size_t rscr = 0, part = 0;                                  // device-only
  size_t bst = 0, olen = 0, out = 0;                          // outputs, from out_base()

  // A borrowed image: plan_handle for each handle, and the sizes they add up to.
  int plan(const uint8_t* file, uint64_t file_len, const uint64_t* off, const uint64_t* size,
           uint32_t count) {
    reset(count, false);
    file_ = file, off_ = off, size_ = size;
    plans.resize(n);
    for (uint32_t j = 0; j < n; ++j) {
      LGS_TRY(plan_handle(file, file_len, off[j], size[j], &plans[j]));
      if (plans[j].in_file) img += align_up((size_t)size[j] + LGS_TRAILER_SIZE, 16);
      outb += align_up(plans[j].cap, 16);
      if (plans[j].cap > max_cap) max_cap = plans[j].cap;
    }
    return LGS_OK;
  }
  // A resident image: launch_block_plan's sums, as read back from its info.
  void plan_resident(uint32_t count, size_t out_bytes, uint32_t max_out_cap) {
    reset(count, true);
    outb = out_bytes;
    max_cap = max_out_cap;
  }

  // (A resident image: only the output offsets, which the device writes.)
  void take_upload(Layout& L) {
    blk = L.take(resident_ ? 0 : img + 32);
    hoff = L.take(resident_ ? 0 : 8 * (size_t)n);
    hsize = L.take(resident_ ? 0 : 8 * (size_t)n);
    ooff = L.take(8 * (size_t)n);
    ocap = L.take(resident_ ? 0 : 4 * (size_t)n);
  }
  void take_scratch(Layout& L) {
    rscr = L.take(R.total);
    part = L.take(resident_ ? 8 * scan_parts(n) + 8 : 0);
  }
  // The statuses first: a caller that downloads them ends its download run
  // at bst + n.  An output side that lives elsewhere (the opened table keeps
  // what the read leaves) sets bst, olen and out itself, as offsets from the
  // base it gives to stage.
  void take_output(Layout& L) {
    bst = L.take(n);
    olen = L.take(4 * (size_t)n);
    out = L.take(outb + 16);
  }

  // Borrowed: the handles' byte ranges packed 16-aligned at h + blk
  // (lgs_table_read_host's layout: a handle outside the file points past the
  // image, so the device reports the truncated read), the handle arrays and
  // each block's 16-aligned output slot from `out` on.  h is the pinned arena,
  // e the device one, o the outputs' base when that is not e.
  void stage(uint8_t* h, uint8_t* e, uint8_t* o = nullptr) {
    uint64_t* ho = (uint64_t*)(h + hoff);
    uint64_t* hs = (uint64_t*)(h + hsize);
    uint64_t* oo = (uint64_t*)(h + ooff);
    uint32_t* oc = (uint32_t*)(h + ocap);
    size_t ba = 0, oa = out;
    for (uint32_t j = 0; j < n; ++j) {
      hs[j] = size_[j];
      ho[j] = plans[j].in_file ? ba : ~0ull;
      if (plans[j].in_file) ba += align_up((size_t)size_[j] + LGS_TRAILER_SIZE, 16);
      oo[j] = oa;
      oc[j] = plans[j].cap;
      oa += align_up(plans[j].cap, 16);
    }
    for (uint32_t j = 0; j < n; ++j)
      if (ho[j] == ~0ull) ho[j] = ba + 16 + 1;
    par_for(n, ba, [&](uint32_t j0, uint32_t j1) {
      for (uint32_t j = j0; j < j1; ++j)
        if (ho[j] <= ba)
          memcpy(h + blk + ho[j], file_ + off_[j], (size_t)size_[j] + LGS_TRAILER_SIZE);
    });
    bind(e, o ? o : e, e + blk, img + 16, (const uint64_t*)(e + hoff), (const uint64_t*)(e + hsize),
         (const uint32_t*)(e + ocap));
  }
  // Resident: the handles are on the device, and so is what
  // launch_block_plan wrote for them, each block's cap and 16-aligned room;
  // the rooms' running sum from `out` on gives the output slots.
  int bind_resident(uint8_t* e, const uint8_t* d_image, uint64_t file_len, const uint64_t* d_off,
                    const uint64_t* d_size, const uint32_t* d_cap, const uint32_t* d_room,
                    hipStream_t s) {
    bind(e, e, d_image, file_len, d_off, d_size, d_cap);
    LGS_HIP(launch_scan(2, nullptr, d_room, (uint64_t*)(e + part), out, (uint64_t*)(e + ooff),
                        nullptr, n, s));
    return LGS_OK;
  }

  int read(int verify, hipStream_t s) const {
    return table_read(d_file_, file_len_, d_hoff_, d_hsize_, n, verify, o_, d_out_off(), d_ocap_,
                      max_cap, d_out_len(), d_status(), e_ + rscr, R, s);
  }
  // Block j decoded at out_base() + d_out_off()[j], d_out_len()[j] bytes.
  uint8_t* out_base() const { return o_; }
  uint64_t* d_out_off() const { return (uint64_t*)(e_ + ooff); }
  uint32_t* d_out_len() const { return (uint32_t*)(o_ + olen); }
  uint8_t* d_status() const { return o_ + bst; }

 private:
  void reset(uint32_t count, bool resident) {
    n = count;
    resident_ = resident;
    R = ReadScratch(n);
    img = outb = 0;
    max_cap = 0;
  }
  void bind(uint8_t* e, uint8_t* o, const uint8_t* d_file, uint64_t file_len, const uint64_t* d_hoff,
            const uint64_t* d_hsize, const uint32_t* d_ocap) {
    e_ = e, o_ = o;
    d_file_ = d_file, file_len_ = file_len, d_hoff_ = d_hoff, d_hsize_ = d_hsize, d_ocap_ = d_ocap;
  }
  bool resident_ = false;
  const uint8_t* file_ = nullptr;                   // the borrowed image and its handles
  const uint64_t *off_ = nullptr, *size_ = nullptr;
  uint8_t *e_ = nullptr, *o_ = nullptr;             // once bound: the arena, the outputs' base
  const uint8_t* d_file_ = nullptr;                 // and table_read's inputs
  uint64_t file_len_ = 0;
  const uint64_t *d_hoff_ = nullptr, *d_hsize_ = nullptr;
  const uint32_t* d_ocap_ = nullptr;
};

// What a get's second half leaves per query, inside its arena: downloads
// (koff .. verdict), then device-only.
struct GetResults {
  size_t koff, voff, called, fst, verdict, len, sst, vsrc, vn, part;
  void take(Layout& L, uint32_t nq) {
    koff = L.take(8 * ((size_t)nq + 1));
    voff = L.take(8 * ((size_t)nq + 1));
    called = L.take(nq);
    fst = L.take(nq);
    verdict = L.take(nq);
    len = L.take(4 * (size_t)nq);
    sst = L.take(nq);
    vsrc = L.take(8 * (size_t)nq);
    vn = L.take(4 * (size_t)nq);
    part = L.take(8 * scan_parts(nq) + 8);
  }
};

// A table that did not open: every query fails with its status (on the
// device: launch_get_fail).
int get_fail_all(uint8_t st, uint32_t nq, uint8_t* called, uint8_t* status, uint8_t* verdict,
                 uint64_t* out_key_off, uint64_t* out_val_off) {
  for (uint32_t q = 0; q < nq; ++q) {
    called[q] = 0;
    status[q] = st;
    if (verdict) verdict[q] = kGetNotFound;
    out_key_off[q + 1] = out_val_off[q + 1] = 0;
  }
  return LGS_OK;
}

// Phase C of a host get: keys, values and verdicts gathered into a packed
// device buffer, which comes down with the value offsets and the verdicts.
// ga is complete but for `out`; ga.verdict is where the device writes the
// verdicts (null: none wanted, and the host's are all kGetNotFound).
// pack_empty: launch_pack even when there are no result bytes.
int get_host_tail(GatherArgs ga, uint64_t total, bool pack_empty, uint8_t* out,
                  uint64_t* out_val_off, uint8_t* verdict, hipStream_t s) {
  std::unique_ptr<Scratch> packed;
  LGS_TRY(scratch_alloc(&packed, (size_t)total + 16, s, "the results"));
  ga.out = (uint8_t*)packed->get();
  LGS_HIP(launch_get_gather(ga, s));
  if (total || pack_empty)
    LGS_HIP(launch_pack(ga.blocks, ga.val_src, ga.val_n, ga.out, ga.out_val_off, ga.nq, s));
  if (total) LGS_HIP(hipMemcpyAsync(out, ga.out, (size_t)total, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(out_val_off, ga.out_val_off, 8 * ((size_t)ga.nq + 1),
                         hipMemcpyDeviceToHost, s));
  if (ga.verdict) LGS_HIP(hipMemcpyAsync(verdict, ga.verdict, ga.nq, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  if (verdict && !ga.verdict) memset(verdict, kGetNotFound, ga.nq);
  return LGS_OK;
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
  if (open_st != LGS_ST_OK)
    return get_fail_all(open_st, nq, called, status, verdict, out_key_off, out_val_off);
  const bool want_filter = h2_off[1] != ~0ull;
  const uint32_t n2 = want_filter ? 2u : 1u;
  BlockRead A;
  LGS_TRY(A.plan(file, file_len, h2_off, h2_size, n2));
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  hipStream_t s = c.stream;

  // -- A: index (and filter) block, the index seek, the handles, the filter.
  Layout L;  // uploads | downloads | device-only
  const size_t o_keys = L.take(kb + 16);
  const size_t o_koff = L.take(8 * (size_t)nq);
  const size_t o_klen = L.take(4 * (size_t)nq);
  A.take_upload(L);
  const size_t o_zero = L.take(8);
  const size_t up_end = L.at;
  const size_t o_state = L.take(nq);           // downloads, contiguous
  const size_t o_match = L.take(nq);
  const size_t o_sst = L.take(nq);
  const size_t o_qhoff = L.take(8 * (size_t)nq);
  const size_t o_qhsize = L.take(8 * (size_t)nq);
  A.take_output(L);
  const size_t down_end = A.bst + n2;          // the two blocks' statuses come down too
  const size_t o_epos = L.take(4 * (size_t)nq);
  const size_t o_fkl = L.take(4 * (size_t)nq);
  const size_t o_vpos = L.take(4 * (size_t)nq);
  const size_t o_vlen = L.take(4 * (size_t)nq);
  const size_t o_rpos = L.take(lgs_block_seek_scratch(nq));
  A.take_scratch(L);
  LGS_TRY(ctx_reserve(c, L.at, down_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  stage_keys(keys, key_off, key_len, nq, h + o_keys, (uint64_t*)(h + o_koff),
             (uint32_t*)(h + o_klen));
  *(uint64_t*)(h + o_zero) = 0;
  A.stage(h, d);
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, s));
  const uint8_t* d_keys = d + o_keys;
  const uint64_t* d_koff = (const uint64_t*)(d + o_koff);
  const uint32_t* d_klen = (const uint32_t*)(d + o_klen);
  uint32_t* d_epos = (uint32_t*)(d + o_epos);
  uint32_t* d_fkl = (uint32_t*)(d + o_fkl);
  uint32_t* d_vpos = (uint32_t*)(d + o_vpos);
  uint32_t* d_vlen = (uint32_t*)(d + o_vlen);
  uint32_t* d_rpos = (uint32_t*)(d + o_rpos);
  LGS_TRY(A.read(paranoid_checks, s));
  // The index block stays where the read put it: block 0 of the seek.
  const uint8_t* d_index = d + A.out;
  const SeekArgs ia{d_index, (const uint64_t*)(d + o_zero), A.d_out_len(), A.d_status(), 1, nullptr,
                    d_keys, d_koff, d_klen, nq, (uint32_t)internal_keys, d_epos, d_fkl, d_vpos,
                    d_vlen, d + o_sst, d_rpos, nullptr, nullptr, nullptr};
  LGS_HIP(launch_block_seek(ia, s));
  LGS_HIP(launch_get_handles(d_index, d_epos, d_vpos, d_vlen, nq, (uint64_t*)(d + o_qhoff),
                             (uint64_t*)(d + o_qhsize), d + o_state, s));
  if (want_filter) {
    // The block's length as the host knows it; a filter block that does not
    // read is dropped below (table.c:71-72), whatever was matched in it.
    LGS_HIP(launch_filter_block_match(d_index + align_up(A.plans[0].cap, 16), A.plans[1].cap,
                                      (const uint64_t*)(d + o_qhoff), d_keys, d_koff, d_klen,
                                      internal_keys ? 8u : 0u, d + o_match, nq, s));
  }
  LGS_HIP(hipMemcpyAsync(h + o_state, d + o_state, down_end - o_state, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));   // the read-back that sizes and de-duplicates the block read

  // -- B: the distinct data blocks the surviving queries name.
  const bool filter = want_filter && h[A.bst + 1] == LGS_ST_OK;
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
  BlockRead D;
  LGS_TRY(D.plan(file, file_len, b_off.data(), b_size.data(), nb));
  Layout B;  // uploads | downloads | device-only
  D.take_upload(B);
  const size_t p_qblock = B.take(4 * (size_t)nq);
  const size_t p_pre = B.take(nq);
  const size_t pin_b = B.at;
  GetResults P;
  P.take(B, nq);
  D.take_scratch(B);
  D.take_output(B);
  LGS_TRY(ctx_reserve(c, 0, pin_b));
  h = c.h_buf;
  std::unique_ptr<Scratch> arena;
  LGS_TRY(scratch_alloc(&arena, B.at, s, "the block read"));
  uint8_t* e = (uint8_t*)arena->get();
  D.stage(h, e);
  memcpy(h + p_qblock, qblock.data(), 4 * (size_t)nq);
  memcpy(h + p_pre, pre.data(), nq);
  LGS_HIP(hipMemcpyAsync(e, h, pin_b, hipMemcpyHostToDevice, s));
  if (nb) LGS_TRY(D.read(verify_checksums, s));
  const uint32_t* d_qblock = (const uint32_t*)(e + p_qblock);
  const SeekArgs da{D.out_base(), D.d_out_off(), D.d_out_len(), D.d_status(), nb, d_qblock, d_keys,
                    d_koff, d_klen, nq, (uint32_t)internal_keys, d_epos, d_fkl, d_vpos, d_vlen,
                    e + P.sst, d_rpos, nullptr, nullptr, nullptr};
  LGS_HIP(launch_block_seek(da, s));
  LGS_HIP(launch_get_lens(d_qblock, e + p_pre, d_epos, d_fkl, d_vlen, e + P.sst, nq, e + P.called,
                          e + P.fst, (uint32_t*)(e + P.len), s));
  uint64_t* d_okoff = (uint64_t*)(e + P.koff);
  LGS_HIP(launch_scan(2, nullptr, (const uint32_t*)(e + P.len), (uint64_t*)(e + P.part), 0, d_okoff,
                      d_okoff + nq, nq, s));
  LGS_HIP(hipMemcpyAsync(out_key_off, d_okoff, 8 * ((size_t)nq + 1), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(called, e + P.called, nq, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(status, e + P.fst, nq, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  for (uint32_t q = 0; q < nq; ++q)
    if (status[q] == LGS_ST_NOSPACE) status[q] = LGS_ST_CORRUPT;   // plan_handle's cap
  const uint64_t total = out_key_off[nq];
  *out_needed = (size_t)total;
  if (total > out_cap)
    return fail(LGS_ENOSPC, "results take %llu bytes, out_cap %zu", (unsigned long long)total,
                out_cap);

  // -- C: keys, values and verdicts into the packed output.
  const GatherArgs ga{D.out_base(), D.d_out_off(), d_qblock, d_keys, d_koff, d_klen, e + P.called,
                      d_epos, d_rpos, d_fkl, d_vpos, d_vlen, nq, nullptr, d_okoff,
                      (uint64_t*)(e + P.voff), (uint64_t*)(e + P.vsrc), (uint32_t*)(e + P.vn),
                      verdict && internal_keys ? e + P.verdict : nullptr};
  return get_host_tail(ga, total, true, out, out_val_off, verdict, s);
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
    return get_fail_all(t->status, nq, io.called, io.status, io.verdict, io.out_key_off,
                        io.out_val_off);
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
  std::unique_ptr<Scratch> first;
  LGS_TRY(scratch_alloc(&first, G.total, s, "the queries"));
  uint8_t* d = (uint8_t*)first->get();
  const uint8_t* d_keys = io.keys;
  const uint64_t* d_koff = io.key_off;
  const uint32_t* d_klen = io.key_len;
  if (!io.dev) {
    stage_keys(io.keys, io.key_off, io.key_len, nq, h + G.keys, (uint64_t*)(h + G.koff),
               (uint32_t*)(h + G.klen));
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
  BlockRead D;
  std::vector<uint64_t> b_off, b_size;
  if (t->resident) {
    if (info[3])
      return fail(LGS_EINVAL, "a block of 2^31 bytes or more: under 2^31 supported");
    D.plan_resident(nb, (size_t)info[1], (uint32_t)info[2]);
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
    LGS_TRY(D.plan(t->file, t->file_len, b_off.data(), b_size.data(), nb));
  }
  Layout B;  // uploads (a borrowed image only) | device-only
  D.take_upload(B);
  const size_t pin_b = B.at;
  GetResults P;
  P.take(B, nq);
  D.take_scratch(B);
  D.take_output(B);
  std::unique_ptr<Scratch> arena;
  LGS_TRY(scratch_alloc(&arena, B.at, s, "the block read"));
  uint8_t* e = (uint8_t*)arena->get();
  if (t->resident) {
    LGS_TRY(D.bind_resident(e, t->d + t->o_img, t->file_len, d_boff, d_bsize, d_ocap,
                            (const uint32_t*)(d + G.room), s));
  } else {
    LGS_TRY(ctx_reserve(c, 0, pin_b + 64));
    h = c.h_buf;
    D.stage(h, e);
    LGS_HIP(hipMemcpyAsync(e, h, pin_b, hipMemcpyHostToDevice, s));
  }
  if (nb) LGS_TRY(D.read(verify_checksums, s));
  const SeekArgs da{D.out_base(), D.d_out_off(), D.d_out_len(), D.d_status(), nb, d_qblock, d_keys,
                    d_koff, d_klen, nq, internal_keys, d_epos, d_fkl, d_vpos, d_vlen, e + P.sst,
                    d_rpos, nullptr, nullptr, nullptr};
  LGS_HIP(launch_block_seek(da, s));
  uint8_t* d_called = io.dev ? io.called : e + P.called;
  uint8_t* d_fst = io.dev ? io.status : e + P.fst;
  LGS_HIP(launch_get_lens(d_qblock, d + G.pre, d_epos, d_fkl, d_vlen, e + P.sst, nq, d_called,
                          d_fst, (uint32_t*)(e + P.len), s));
  LGS_HIP(launch_nospace_is_corrupt(d_fst, nq, s));                // plan_handle's cap
  uint64_t* d_okoff = io.dev ? io.out_key_off : (uint64_t*)(e + P.koff);
  uint64_t* d_ovoff = io.dev ? io.out_val_off : (uint64_t*)(e + P.voff);
  LGS_HIP(launch_scan(2, nullptr, (const uint32_t*)(e + P.len), (uint64_t*)(e + P.part), 0, d_okoff,
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

  // -- C: keys, values and verdicts into the packed output (a host call:
  // into a packed device buffer that comes down, get_host_tail).
  uint8_t* d_verdict = io.dev ? io.verdict : e + P.verdict;
  const GatherArgs ga{D.out_base(), D.d_out_off(), d_qblock, d_keys, d_koff, d_klen, d_called,
                      d_epos, d_rpos, d_fkl, d_vpos, d_vlen, nq, io.out, d_okoff, d_ovoff,
                      (uint64_t*)(e + P.vsrc), (uint32_t*)(e + P.vn),
                      io.verdict && internal_keys ? d_verdict : nullptr};
  if (!io.dev) return get_host_tail(ga, total, false, io.out, io.out_val_off, io.verdict, s);
  LGS_HIP(launch_get_gather(ga, s));
  if (total) LGS_HIP(launch_pack(ga.blocks, ga.val_src, ga.val_n, ga.out, d_ovoff, nq, s));
  // The scratch is freed on the stream behind the work that uses it.
  if (io.verdict && !internal_keys) LGS_HIP(hipMemsetAsync(io.verdict, kGetNotFound, nq, s));
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
  BlockRead A;
  LGS_TRY(A.plan(file, file_len, h2_off, h2_size, n2));
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  hipStream_t s = c.stream;
  // The index and filter block through table_read, once; what it leaves
  // stays: the decoded blocks, their lengths and statuses go to the handle's
  // own memory, not to the stage's arena.
  Layout L;  // uploads | device-only
  A.take_upload(L);
  const size_t up_end = L.at;
  A.take_scratch(L);
  Layout T;
  A.out = T.take(A.outb + 16);
  t->o_filter = align_up(A.plans[0].cap, 16);
  A.olen = t->o_olen = T.take(8);
  A.bst = t->o_bst = T.take(2);
  t->o_zero = T.take(8);
  t->o_img = T.take(resident ? (size_t)file_len + 16 : 0);
  t->d_bytes = T.at;
  LGS_TRY(ctx_reserve(c, 0, up_end + 64));
  uint8_t* h = c.h_buf;
  t->stream = s;
  std::unique_ptr<Scratch> stage;
  LGS_TRY(scratch_alloc(&t->mem, t->d_bytes, s, "the opened table"));
  LGS_TRY(scratch_alloc(&stage, L.at, s, "opening the table"));
  t->d = (uint8_t*)t->mem->get();
  uint8_t* d = (uint8_t*)stage->get();
  A.stage(h, d, t->d);
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, s));
  LGS_HIP(hipMemsetAsync(t->d + t->o_olen, 0, t->o_img - t->o_olen, s));
  if (resident) {
    if (file_len) LGS_HIP(hipMemcpyAsync(t->d + t->o_img, file, (size_t)file_len,
                                         hipMemcpyHostToDevice, s));
    LGS_HIP(hipMemsetAsync(t->d + t->o_img + file_len, 0, 16, s));
  }
  LGS_TRY(A.read(paranoid_checks, s));
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
    t->filter_len = want_filter ? A.plans[1].cap : 0;
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

// The second half of a host scan, after the read-back of the counts: the n
// entries (of `walked`) emitted into one device arena, which comes down in
// one copy.  pb: the count's scratch, laid out by B.
int entries_emit_host(Ctx& c, hipStream_t s, const EntriesIn& in, uint8_t* pb,
                      const EntriesBlockLayout& B, uint64_t walked, uint64_t n, uint64_t kb,
                      uint64_t vb, uint8_t* keys, uint64_t* key_off, uint32_t* key_len, uint8_t* vals,
                      uint64_t* val_off, uint32_t* val_len) {
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
  std::unique_ptr<Scratch> arena;
  LGS_TRY(scratch_alloc(&arena, O.at, s, "the entries"));
  uint8_t* e = (uint8_t*)arena->get();
  LGS_HIP(launch_entries_emit(in, entries_scratch(pb, B, e + q_scr, &E), walked, (uint32_t)n,
                              e + q_keys, (uint64_t*)(e + q_koff), (uint32_t*)(e + q_klen),
                              e + q_vals, (uint64_t*)(e + q_voff), (uint32_t*)(e + q_vlen), s));
  LGS_TRY(ctx_reserve(c, 0, q_end));
  const uint8_t* h = c.h_buf;
  LGS_HIP(hipMemcpyAsync(c.h_buf, e, q_end, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  memcpy(keys, h + q_keys, (size_t)kb);
  memcpy(vals, h + q_vals, (size_t)vb);
  memcpy(key_off, h + q_koff, 8 * ((size_t)n + 1));
  memcpy(val_off, h + q_voff, 8 * ((size_t)n + 1));
  memcpy(key_len, h + q_klen, 4 * (size_t)n);
  memcpy(val_len, h + q_vlen, 4 * (size_t)n);
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
  return entries_emit_host(c, s, in, d + o_scr, B, walked, n, kb, vb, keys, key_off, key_len, vals,
                           val_off, val_len);
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
  std::unique_ptr<Scratch> tmp;
  LGS_TRY(scratch_alloc(&tmp, T.total, s, "the index entries"));
  uint8_t* d = (uint8_t*)tmp->get();
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
  LGS_TRY(scratch_alloc(&t->list_mem, F.at, t->stream, "the index entries"));
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
    if (t->list_rc != LGS_OK) snprintf(t->list_err, sizeof t->list_err, "%s", lgs_last_error());
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
    LGS_TRY(scratch_alloc(&seek_mem, S.at, s, "the seek"));
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
      LGS_TRY(scratch_alloc(&side_mem, T.total, s, "the index entries"));
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
  BlockRead D;
  std::unique_ptr<Scratch> plan_mem;
  uint8_t* pd = nullptr;
  if (t->resident) {
    LGS_TRY(ctx_reserve(c, 0, 64));
    uint8_t* h = c.h_buf;
    LGS_TRY(scratch_alloc(&plan_mem, P.at, s, "the blocks' plan"));
    pd = (uint8_t*)plan_mem->get();
    LGS_HIP(launch_plan_info((uint64_t*)(pd + p_info), nb, s));
    LGS_HIP(launch_block_plan(t->d + t->o_img, t->file_len, dw_hoff, dw_hsize, nb,
                              (uint32_t*)(pd + p_ocap), (uint32_t*)(pd + p_room),
                              (uint64_t*)(pd + p_info), s));
    LGS_HIP(hipMemcpyAsync(h, pd + p_info, 32, hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));   // the read-back that sizes the block read
    const uint64_t* info = (const uint64_t*)h;
    if (info[3]) return fail(LGS_EINVAL, "a block of 2^31 bytes or more: under 2^31 supported");
    D.plan_resident(nb, (size_t)info[1], (uint32_t)info[2]);
  } else {
    LGS_TRY(D.plan(t->file, t->file_len, w_hoff, w_hsize, nb));
  }
  Layout B;  // uploads (a borrowed image only) | downloads | device-only
  D.take_upload(B);
  const size_t p_state = B.take(nb);
  const size_t pin_b = B.at;
  const size_t p_cnt = B.take(8 * kEntryCounts);      // downloads
  const size_t p_head = B.take(16);
  const size_t p_first = B.take(4 * ((size_t)nb + 1));
  const size_t p_st = B.take(nb);
  const size_t down_end = B.at;
  const size_t p_wf = B.take(4 * (size_t)nb);
  const size_t p_ef = B.take(4 * (size_t)nb);
  const size_t p_ef_end = B.at;
  const size_t p_escr = B.take(EB.total);
  D.take_scratch(B);
  D.take_output(B);
  LGS_TRY(ctx_reserve(c, 0, std::max(pin_b, down_end - p_cnt) + 64));
  uint8_t* h = c.h_buf;
  std::unique_ptr<Scratch> arena;
  LGS_TRY(scratch_alloc(&arena, B.at, s, "the block read"));
  uint8_t* e = (uint8_t*)arena->get();
  const uint8_t* d_state = dw_state;
  if (t->resident) {
    LGS_TRY(D.bind_resident(e, t->d + t->o_img, t->file_len, dw_hoff, dw_hsize,
                            (const uint32_t*)(pd + p_ocap), (const uint32_t*)(pd + p_room), s));
  } else {
    D.stage(h, e);
    memcpy(h + p_state, w_state, nb);
    LGS_HIP(hipMemcpyAsync(e, h, pin_b, hipMemcpyHostToDevice, s));
    d_state = e + p_state;
  }
  LGS_TRY(D.read(verify_checksums, s));
  LGS_HIP(launch_scan_status(d_state, D.d_status(), nb, s));
  const uint32_t* d_wf = nullptr;
  const uint32_t* d_ef = nullptr;
  if (io.has_start) {
    // ldb_twoiter_seek's data seek: a fresh iterator on the window's first
    // block; the scan goes on from the entry it found, in the restart run it
    // chose.
    LGS_HIP(hipMemsetAsync(e + p_wf, 0xff, p_ef_end - p_wf, s));
    const SeekArgs da{D.out_base(), D.d_out_off(), D.d_out_len(), D.d_status(), nb, nullptr, d_start, d_start_off, d_start_len, 1, internal_keys,
                      (uint32_t*)(sk + s_epos), (uint32_t*)(sk + s_fkl), (uint32_t*)(sk + s_vpos),
                      (uint32_t*)(sk + s_vlen), sk + s_sst, (uint32_t*)(sk + s_rpos), nullptr,
                      nullptr, nullptr};
    LGS_HIP(launch_block_seek(da, s));
    LGS_HIP(launch_scan_seek_apply((const uint32_t*)(sk + s_epos), (const uint32_t*)(sk + s_rpos),
                                   sk + s_sst, (uint32_t*)(e + p_wf), (uint32_t*)(e + p_ef),
                                   D.d_status(), s));
    d_wf = (const uint32_t*)(e + p_wf);
    d_ef = (const uint32_t*)(e + p_ef);
  }

  // -- C: the entries (§2's two calls around the read-back of the counts).
  const EntriesIn in{D.out_base(), D.d_out_off(), D.d_out_len(), D.d_status(), nb, d_wf, d_ef,
                     internal_keys};
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
  if (!io.dev)
    return entries_emit_host(c, s, in, e + p_escr, EB, walked, n, kb, vb, io.keys, io.key_off,
                             io.key_len, io.vals, io.val_off, io.val_len);
  const EntriesEntryLayout EE(walked, n);
  std::unique_ptr<Scratch> second;
  LGS_TRY(scratch_alloc(&second, EE.total, s, "the entries"));
  // The scratch is freed on the stream behind the work that uses it.
  LGS_HIP(launch_entries_emit(in, entries_scratch(e + p_escr, EB, (uint8_t*)second->get(), &EE),
                              walked, (uint32_t)n, io.keys, io.key_off, io.key_len, io.vals,
                              io.val_off, io.val_len, s));
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

}  // extern "C"
