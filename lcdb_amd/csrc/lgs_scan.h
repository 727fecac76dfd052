// lgs_scan.h -- host-side launch interface of the forward scan (lgs_scan.hip,
// DESIGN §4.7): the entries of decoded blocks out in the builder's layout, and
// the opened table's index entry list.
#pragma once

#include "lgs_launch.h"

namespace lgs {

constexpr uint32_t kNoOffset = 0xffffffffu;   // walk_from / emit_from: not given
constexpr uint32_t kNoLink = 0xffffffffu;     // an entry with shared = 0 has no link
constexpr uint32_t kEntryCounts = 4;          // {entries, key bytes, value bytes, longest key}

// Decoded blocks as lgs_table_read_dev leaves them (SeekArgs' first half);
// walk_from / emit_from (null, or kNoOffset per block: not given): where the
// walk of block b begins instead of restart[0], and the first offset whose
// entry is delivered.
struct EntriesIn {
  const uint8_t* blocks; const uint64_t* block_off; const uint32_t* block_len;
  const uint8_t* block_status; uint32_t nblocks;
  const uint32_t* walk_from; const uint32_t* emit_from; uint32_t internal;
};

// Device scratch, kept from the count to the emit.  Per block: the entries the
// walk parses (wcnt) and those it delivers (dcnt), their exclusive scans, and
// head = {entries walked, entries delivered}.  Per walked entry m: src (offset
// of its key delta in its block), shared, link (the nearest earlier walked
// entry whose shared is smaller, kNoLink when shared = 0).  Per delivered
// entry i: its block and its walked number.  part: launch_scan's.
struct EntriesScratch {
  uint64_t* head; uint32_t* wcnt; uint32_t* dcnt; uint64_t* wfirst; uint64_t* dfirst;
  uint64_t* part;
  uint32_t* src; uint32_t* shared; uint32_t* link; uint32_t* eblk; uint32_t* emeta;
};

// The header walk, first run: status[b], entry_first (nblocks + 1), counts
// (kEntryCounts u64), and the per-block half of the scratch.
hipError_t launch_entries_count(const EntriesIn& in, const EntriesScratch& w, uint32_t* entry_first,
                                uint8_t* status, uint64_t* counts, hipStream_t s);
// The second run and the copy: n delivered entries (counts[0]) into keys /
// vals; key_off and val_off get n + 1 values, key_len and val_len n.  wcap:
// the walked entries the scratch has room for (head[0] at least).
hipError_t launch_entries_emit(const EntriesIn& in, const EntriesScratch& w, uint64_t wcap,
                               uint32_t n, uint8_t* keys, uint64_t* key_off, uint32_t* key_len, uint8_t* vals,
                               uint64_t* val_off, uint32_t* val_len, hipStream_t s);

// ---- the opened table's index entry list ----
//
// The index block's entries in walk order: pos (the entry's offset), the
// handle its value decodes to (state 1) or ~0 / 0 (state 2: no handle).
// info (4 u64): {entries, the walk's end status, 1 = the slots disagreed, 0}.
struct IndexList {
  uint32_t* pos; uint64_t* hoff; uint64_t* hsize; uint8_t* state; uint64_t* info;
};
// A lane per restart slot; exact when info[2] stays 0.  cap: room of the
// arrays, at least len / 4 + 1.
hipError_t launch_index_slots(const uint8_t* index, uint32_t len, uint32_t internal, uint32_t cap,
                              const IndexList& out, hipStream_t s);
// The serial walk, exact for any contents: from restart[0] (from = kNoOffset),
// or from an entry a seek has found (its `shared` is not checked again).
// cap: at least len / 3 + 1.
hipError_t launch_index_walk(const uint8_t* index, uint32_t len, uint32_t internal, uint32_t from,
                             uint32_t cap, const IndexList& out, hipStream_t s);

// One window's block statuses after the read: an entry without a handle is
// corrupt (table.c:244-245), and the room's cap stands for corrupt contents.
hipError_t launch_scan_status(const uint8_t* state, uint8_t* block_status, uint32_t nb,
                              hipStream_t s);
// The seek's outcome in the window's first block: walk from the restart run
// the seek chose and deliver from the entry it found; no entry: nothing is
// delivered and a status other than OK becomes the block's.  walk_from and
// emit_from are kNoOffset everywhere else (set beforehand).
hipError_t launch_scan_seek_apply(const uint32_t* entry_pos, const uint32_t* restart_pos,
                                  const uint8_t* seek_status, uint32_t* walk_from,
                                  uint32_t* emit_from, uint8_t* block_status, hipStream_t s);
// info = {nb, 0, 0, 0} for launch_block_plan.
hipError_t launch_plan_info(uint64_t* info, uint32_t nb, hipStream_t s);

}  // namespace lgs
