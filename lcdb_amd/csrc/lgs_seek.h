// lgs_seek.h -- host-side launch interface of the block seek and the batched
// table Get (lgs_seek.hip), used by the runtime (lgs_api.cpp).
#pragma once

#include "lgs_launch.h"

namespace lgs {

constexpr uint32_t kNoEntry = 0xffffffffu;   // entry_pos of a query without an entry
constexpr uint32_t kNoBlock = 0xffffffffu;   // a query that names no block

// nq queries: query q seeks key q in block qblock[q] (>= nblocks: no block,
// which gives no entry and kStOk).  Block b = blocks[block_off[b] ..
// + block_len[b]); block_status (may be null) as the C ABI states it.
struct SeekArgs {
  const uint8_t* blocks; const uint64_t* block_off; const uint32_t* block_len;
  const uint8_t* block_status; uint32_t nblocks;
  const uint32_t* qblock;
  const uint8_t* keys; const uint64_t* key_off; const uint32_t* key_len;
  uint32_t nq; uint32_t internal;
  uint32_t* entry_pos; uint32_t* found_key_len; uint32_t* val_pos; uint32_t* val_len;
  uint8_t* status;
  uint32_t* restart_pos;   // scratch, nq: where the found entry's restart run starts
  // The found key, unless key_out is null.
  uint8_t* key_out; const uint64_t* key_out_off; const uint32_t* key_out_cap;
};
hipError_t launch_block_seek(const SeekArgs& a, hipStream_t s);

// ldb_handle_import (format.c:66-80) of each index entry the seek found, in
// block 0 of `blocks`: state 0 = no entry, 1 = a handle (hoff, hsize), 2 = an
// entry whose value is no handle.
hipError_t launch_get_handles(const uint8_t* index_block, const uint32_t* entry_pos,
                              const uint32_t* val_pos, const uint32_t* val_len, uint32_t nq,
                              uint64_t* hoff, uint64_t* hsize, uint8_t* state, hipStream_t s);

// table.c:345-359 per query after the data-block seek: called, the status
// (pre[q] for a query that named no block) and the bytes of its result.
hipError_t launch_get_lens(const uint32_t* qblock, const uint8_t* pre, const uint32_t* entry_pos,
                           const uint32_t* found_key_len, const uint32_t* val_len,
                           const uint8_t* seek_status, uint32_t nq, uint8_t* called,
                           uint8_t* status, uint32_t* out_len, hipStream_t s);

// Verdicts of version_set.c's save_value (LGS_GET_* of the C ABI).
constexpr uint8_t kGetNotFound = 0, kGetFound = 1, kGetDeleted = 2, kGetCorrupt = 3;

// The gather: query q's found key at out + out_key_off[q]; out_val_off[q] and
// the value's source offset and length for launch_pack; its verdict when
// verdict != null (internal keys only).  out_key_off[nq] is the total, copied
// to out_val_off[nq].
struct GatherArgs {
  const uint8_t* blocks; const uint64_t* block_off; const uint32_t* qblock;
  const uint8_t* keys; const uint64_t* key_off; const uint32_t* key_len;
  const uint8_t* called; const uint32_t* entry_pos; const uint32_t* restart_pos;
  const uint32_t* found_key_len; const uint32_t* val_pos; const uint32_t* val_len;
  uint32_t nq;
  uint8_t* out; const uint64_t* out_key_off; uint64_t* out_val_off;
  uint64_t* val_src; uint32_t* val_n; uint8_t* verdict;
};
hipError_t launch_get_gather(const GatherArgs& a, hipStream_t s);

// ---- the opened table's Get (lgs_table_get, lgs_table_get_dev) ----
//
// The distinct blocks of a batch are numbered on the device.  The key is the
// offset of the index entry a query found, not the (offset, size) its value
// decodes to: entries are marked in an array as long as the index block, an
// exclusive scan of the marks ranks them in file order, and two entries that
// carry the same handle count as two blocks.

constexpr uint64_t kTrailerBytes = 5;           // LGS_TRAILER_SIZE
constexpr uint32_t kMaxRoom = 0xfffffff0u;      // the largest 16-aligned room of one block

// pre[q] as lgs_table_get_host's host loop sets it (state 0: the index seek's
// status; 2: corrupt; a filter miss: OK); qblock[q] = the found entry's offset
// for a live query (state 1 and match == null or match[q]), kNoBlock
// otherwise; mark[that offset] = 1.  mark: index_len u32, zeroed beforehand.
hipError_t launch_live_mark(const uint8_t* state, const uint8_t* match, const uint8_t* seek_status,
                            const uint32_t* entry_pos, uint32_t nq, uint32_t index_len,
                            uint8_t* pre, uint32_t* qblock, uint32_t* mark, hipStream_t s);

// After launch_scan(2, ..) of mark into rank: qblock[q] = the rank of the
// entry it held, and that block's handle (get_handles' hoff, hsize of any of
// its queries) at b_off / b_size[rank].
hipError_t launch_qblock(const uint64_t* rank, const uint64_t* hoff, const uint64_t* hsize,
                         uint32_t nq, uint32_t* qblock, uint64_t* b_off, uint64_t* b_size,
                         hipStream_t s);

// Per distinct block j < info[0] (at most `bound`) of the resident image
// file[0, file_len) (+ 16 readable bytes): out_cap[j] = the room its contents
// take (the raw size; a Snappy block's size header, at most 32 * size + 64 and
// kMaxRoom, 0 if it does not parse; 0 for a handle outside the file) and
// room[j] = that, 16-aligned.  info (4 u64, [1..3] zeroed beforehand):
// [1] += the rooms, [2] = their maximum, [3] |= 1 for a handle of 2^31 bytes
// or more inside the file.
hipError_t launch_block_plan(const uint8_t* file, uint64_t file_len, const uint64_t* b_off,
                             const uint64_t* b_size, uint32_t bound, uint32_t* out_cap,
                             uint32_t* room, uint64_t* info, hipStream_t s);

// A table that did not open: called 0, status st, verdict (may be null)
// kGetNotFound, nq + 1 zero offsets each.
hipError_t launch_get_fail(uint32_t nq, uint8_t st, uint8_t* called, uint8_t* status,
                           uint8_t* verdict, uint64_t* out_key_off, uint64_t* out_val_off,
                           hipStream_t s);

// kStNoSpace -> kStCorrupt in status[0, nq).
hipError_t launch_nospace_is_corrupt(uint8_t* status, uint32_t nq, hipStream_t s);

// Host (lgs_table_index.cpp): the footer's index handle and the metaindex's
// filter handle (~0 / 0: none) of a table image; *status = LGS_ST_CORRUPT for
// a short file or a bad footer.
int table_open(const uint8_t* file, uint64_t file_len, int paranoid_checks,
               const char* filter_name, uint64_t* index_off, uint64_t* index_size,
               uint64_t* filter_off, uint64_t* filter_size, uint8_t* status);

}  // namespace lgs
