// lgs_merge.h -- host-side launch interface of the merge of sorted runs
// (lgs_merge.hip): ldb_mergeiter_first + _next until invalid
// (merger.c) over runs in the builder's layout, and compaction's drop rule
// (db_impl.c:1369-1396).
#pragma once

#include "lgs_launch.h"

namespace lgs {

constexpr uint32_t kMergeMaxRuns = 64;
constexpr uint32_t kMergeCounts = 8;   // {kept, key bytes, value bytes, longest key, dropped,
                                       //  first bad run or ~0, forced starts (the version
                                       //  plan, else 0), 0}
constexpr uint32_t kVersionMaxLevels = 5;   // levels L + 2 .. 6 of a compaction at level L

// One run as the kernels see it: lgs_run plus the number of entries before it.
struct MergeRun {
  const uint8_t* keys; const uint64_t* key_off; const uint32_t* key_len;
  const uint8_t* vals; const uint64_t* val_off; const uint32_t* val_len;
  uint32_t n, first;
};

// Device scratch, kept from the plan to the emit.  table / first: the runs
// (first has kMergeMaxRuns + 1 values, n_total from nruns on).  Per entry
// number e (the inputs numbered run after run): erun.  Per position of the
// order being built, ping-pong: the key word and the entry number.  Per
// position of the final order: keep (0 / 1), the kept key and value lengths,
// their exclusive scans (n + 1 values), the addresses of the entry's key and
// value bytes and where it came from (index << 32 | run).  tot: {kept, key
// bytes, value bytes}.  part: launch_scan's.
struct MergeScratch {
  MergeRun* table; uint32_t* first; uint64_t* tot;
  uint8_t* erun; uint64_t* kw[2]; uint32_t* idx[2];
  uint32_t* keep; uint32_t* klen; uint32_t* vlen;
  uint64_t* ksrc; uint64_t* vsrc; uint64_t* from;
  uint64_t* pos; uint64_t* koff; uint64_t* voff; uint64_t* part;
};

struct MergeRule {
  uint32_t internal, drop, drop_deletions;
  uint64_t smallest_snapshot;
};

// The files of the levels below a compaction's output, in
// device memory: file f's smallest and largest internal keys are the s_len /
// l_len bytes at keys + s_off / l_off (keys readable 16 bytes past its end);
// level v is files [first[v], first[v + 1]).  Level 0 of the list is level + 2,
// the grandparents: P is the exclusive prefix sum of its file sizes (its
// count + 1 values), limit is max_grandparent_overlap_bytes.
struct VersionFile {
  uint64_t s_off, l_off;
  uint32_t s_len, l_len;
};
struct VersionDev {
  const uint8_t* keys; const VersionFile* files; const uint64_t* P;
  uint32_t first[kVersionMaxLevels + 1]; uint32_t nlevels;
  uint64_t limit;
};
// Device scratch of the stops, per position of the final order: pg =
// P[files of level + 2 passed by the key], the stop chain's next / ja / jb /
// mark (lgs_block.hip's steps 3 and 4), the marks' scan sid (n + 1); per kept
// entry: cnt, the stops up to and with it, and forced.  part: launch_scan's.
struct VersionScratch {
  uint64_t* pg; uint32_t* next; uint32_t* ja; uint32_t* jb; uint32_t* mark; uint64_t* sid;
  uint32_t* cnt; uint32_t* forced; uint64_t* part;
};

// runs: host array, `first` filled in.  counts: kMergeCounts u64.
hipError_t launch_merge_plan(const MergeRun* runs, uint32_t nruns, uint32_t n,
                             const MergeRule& rule, const MergeScratch& w, uint64_t* counts,
                             hipStream_t s);
// The plan inside a version: internal keys and the drop rule, with
// ldb_compaction_is_base_level_for_key per entry in place of
// rule.drop_deletions, and ldb_compaction_should_stop_before's stops folded
// onto the kept entries (x.forced, counts[6]).
hipError_t launch_merge_plan_version(const MergeRun* runs, uint32_t nruns, uint32_t n,
                                     const MergeRule& rule, const MergeScratch& w,
                                     const VersionDev& v, const VersionScratch& x,
                                     uint64_t* counts, hipStream_t s);
// The kept entries to their places, from the scratch the plan left; key_off
// and val_off get n_out + 1 values.
hipError_t launch_merge_emit(uint32_t n, uint32_t n_out, const MergeScratch& w, uint8_t* keys,
                             uint64_t* key_off, uint32_t* key_len, uint8_t* vals,
                             uint64_t* val_off, uint32_t* val_len, uint32_t* src_run,
                             uint32_t* src_index, hipStream_t s);

}  // namespace lgs
