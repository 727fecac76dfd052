// lgs_block.h -- host-side launch interface of the data-block builder
// (lgs_block.hip), used by the runtime (lgs_api.cpp).
#pragma once

#include "lgs_launch.h"

namespace lgs {

// n sorted entries: key i = keys[key_off[i] .. + key_len[i]), values alike.
struct BlockIn {
  const uint8_t* keys; const uint64_t* key_off; const uint32_t* key_len;
  const uint8_t* vals; const uint64_t* val_off; const uint32_t* val_len;
  uint32_t n;
};
// Device scratch of the builder, kept from the cut to the emit (the arrays
// of DESIGN §4.5): lcp, sh and the two prefixes S (n + 1) and C (ca/cb: the
// passes' ping-pong, block_c_final() says which holds C), next, the doubled
// jumps ja/jb, the marks, their scan bid, and per block the index key's
// length ilen and cut point icut; part: launch_scan's; fs (n + 1): the
// exclusive scan of the forced starts' flags, when there are any.
struct BlockScratch {
  uint32_t* lcp; uint32_t* sh; uint64_t* S; uint64_t* ca; uint64_t* cb;
  uint32_t* next; uint32_t* ja; uint32_t* jb; uint32_t* mark; uint64_t* bid;
  uint32_t* icut; uint32_t* ilen; uint64_t* part; uint64_t* fs;
};
// Outputs of the cut: block_first, raw_off, ikey_off (n + 1 each), raw_len
// (n), counts = {blocks, raw bytes, longest block, index-key bytes}.
struct BlockCut {
  uint32_t* block_first; uint64_t* raw_off; uint32_t* raw_len; uint64_t* ikey_off;
  uint64_t* counts;
};
constexpr uint32_t kBlockCounts = 4;
// 0: C ends in ca, 1: in cb (the parity of the stride-R passes).
int block_c_final(uint32_t n, uint32_t restart_interval);
// trim: 8 for internal keys (separators work on the user key), else 0.
// forced: null, or n flags (device): an entry i > 0 whose flag is set starts a
// block whatever the size of the block before it (a compaction's output file
// closed by ldb_compaction_should_stop_before).
hipError_t launch_block_cut(const BlockIn& in, uint64_t block_size, uint32_t restart_interval,
                            uint32_t trim, const uint32_t* forced, const BlockScratch& w,
                            const BlockCut& out, hipStream_t s);
// The blocks' bytes at raw + raw_off[b] and (ikey != null) the index keys at
// ikey + ikey_off[b], from the scratch the cut left.
hipError_t launch_block_emit(const BlockIn& in, uint32_t restart_interval, uint32_t trim,
                             uint32_t nblocks, const BlockScratch& w, const uint32_t* block_first,
                             const uint64_t* raw_off, const uint32_t* raw_len, uint8_t* raw,
                             const uint64_t* ikey_off, uint8_t* ikey, hipStream_t s);
// The index keys alone, from icut as the cut (or launch_file_plan) left it.
hipError_t launch_block_ikeys(const BlockIn& in, uint32_t trim, uint32_t nblocks,
                              const BlockScratch& w, const uint32_t* block_first,
                              const uint64_t* ikey_off, uint8_t* ikey, hipStream_t s);
// The index block's entries (table_builder.c:229-239): value b =
// ldb_handle_export(hoff[b] - fstart[b], hsize[b]) at val + 20 b
// (format.c:45-63), its offset and length, and key b's length from the
// index-key offsets.  fstart: the start of block b's file in the framed
// stream (null: 0, one file).
hipError_t launch_handle_values(const uint64_t* hoff, const uint64_t* hsize,
                                const uint64_t* fstart, const uint64_t* ikey_off,
                                uint32_t nblocks, uint8_t* val, uint64_t* val_off,
                                uint32_t* val_len, uint32_t* key_len, hipStream_t s);

// Compaction's output files over one framed stream of nb blocks (handles
// hoff / hsize): a file ends after the first block whose framed end lies
// max_size or more past the file's start (db_impl.c:1417-1425).  next, ja,
// jb, mark, fof, flen (u32) and fid, fstart, rel (u64): nb + 1 each, scratch
// of the search and the doubling and per block its file, that file's start,
// its own offset from there and its framed length; per file (nb + 2 each,
// entry [files] the end): file_block, file_entry (u32), file_start, file_ikey
// (u64); count[0] = files.  fflag (u32, nb + 1) and ffs (u64, nb + 2): per
// block the forced flag of its first entry and the flags' exclusive scan.
struct FilePlan {
  uint32_t* next; uint32_t* ja; uint32_t* jb; uint32_t* mark; uint64_t* fid;
  uint32_t* fof; uint64_t* fstart; uint64_t* rel; uint32_t* flen;
  uint32_t* fflag; uint64_t* ffs;
  uint32_t* file_block; uint32_t* file_entry; uint64_t* file_start; uint64_t* file_ikey;
  uint64_t* count;
};
// The plan, after the blocks are framed and before the index keys are
// emitted: it also turns the index key of every file's last block into the
// short successor (icut, ilen in w) and rescans cut.ikey_off / counts[3].
// forced: as launch_block_cut's; a file also ends before a block whose first
// entry is a forced start.
hipError_t launch_file_plan(const BlockIn& in, uint32_t trim, uint32_t nb, const uint64_t* hoff,
                            const uint64_t* hsize, uint64_t max_size, const uint32_t* forced,
                            const BlockScratch& w, const BlockCut& cut, const FilePlan& p,
                            hipStream_t s);
// dst_off[b] = file_off[file of b] + block b's offset in its file.
hipError_t launch_file_place(const FilePlan& p, const uint64_t* file_off, uint64_t* dst_off,
                             uint32_t nb, hipStream_t s);
// The 48-byte footer (format.c:92-106) of handles {hoff, hsize}[0] (metaindex)
// and [1] (index) at image + *end; *file_size = *end + 48.
hipError_t launch_footer(const uint64_t* hoff, const uint64_t* hsize, const uint64_t* end,
                         uint8_t* image, uint64_t* file_size, hipStream_t s);

// out = {first[0], (uint32_t)*total}: the encoded lengths of the table's last
// two blocks (the metaindex block's own, the index block's packed chunks).
hipError_t launch_pair_lens(const uint32_t* first, const uint64_t* total, uint32_t* out,
                            hipStream_t s);

}  // namespace lgs
