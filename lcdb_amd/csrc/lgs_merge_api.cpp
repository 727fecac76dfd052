// lgs_merge_api.cpp -- the C ABI of the merge of sorted runs (lgs_merge_*,
// include/lcdb_gpu_snappy.h) over the kernels of lgs_merge.hip.
#include <string.h>

#include "lgs_host.h"
#include "lgs_merge.h"

using namespace lgs;

namespace {

constexpr uint64_t kMaxEntries = 0x7fffffffu;

// The scratch of one merge of n entries inside one allocation.
struct MergeLayout {
  size_t table, first, tot, erun, kw[2], idx[2], keep, klen, vlen, ksrc, vsrc, from, pos, koff,
      voff, part, total;
  explicit MergeLayout(size_t n) {
    Layout L;
    table = L.take(sizeof(MergeRun) * kMergeMaxRuns);
    first = L.take(4 * (kMergeMaxRuns + 1));
    tot = L.take(32);
    erun = L.take(n);
    for (int k = 0; k < 2; ++k) kw[k] = L.take(8 * n);
    for (int k = 0; k < 2; ++k) idx[k] = L.take(4 * n);
    keep = L.take(4 * n);
    klen = L.take(4 * n);
    vlen = L.take(4 * n);
    ksrc = L.take(8 * n);
    vsrc = L.take(8 * n);
    from = L.take(8 * n);
    pos = L.take(8 * (n + 1));
    koff = L.take(8 * (n + 1));
    voff = L.take(8 * (n + 1));
    part = L.take(8 * scan_parts((uint32_t)n));
    total = L.at;
  }
  MergeScratch at(uint8_t* p) const {
    return MergeScratch{(MergeRun*)(p + table), (uint32_t*)(p + first), (uint64_t*)(p + tot),
                        p + erun, {(uint64_t*)(p + kw[0]), (uint64_t*)(p + kw[1])},
                        {(uint32_t*)(p + idx[0]), (uint32_t*)(p + idx[1])},
                        (uint32_t*)(p + keep), (uint32_t*)(p + klen), (uint32_t*)(p + vlen),
                        (uint64_t*)(p + ksrc), (uint64_t*)(p + vsrc), (uint64_t*)(p + from),
                        (uint64_t*)(p + pos), (uint64_t*)(p + koff), (uint64_t*)(p + voff),
                        (uint64_t*)(p + part)};
  }
};

// The version plan's scratch: the merge's, the stops' arrays (their places
// depend on n alone: lgs_merge_stops_dev finds `forced` without the levels),
// then the levels as one upload [files, up_end).
struct VersionLayout {
  MergeLayout M;
  size_t pg, next, ja, jb, mark, sid, cnt, forced, part, files, P, keys, up_end, total;
  VersionLayout(size_t n, uint64_t nfiles, uint64_t key_bytes) : M(n) {
    Layout L;
    L.at = M.total;
    pg = L.take(8 * n);
    next = L.take(4 * n);
    ja = L.take(4 * n);
    jb = L.take(4 * n);
    mark = L.take(4 * n + 4);
    sid = L.take(8 * (n + 1));
    cnt = L.take(4 * n);
    forced = L.take(4 * n);
    part = L.take(8 * scan_parts((uint32_t)n));
    files = L.take(sizeof(VersionFile) * (size_t)nfiles);
    P = L.take(8 * ((size_t)nfiles + 1));
    keys = L.take((size_t)key_bytes + 16);
    up_end = L.at;
    total = L.at;
  }
  VersionScratch at(uint8_t* p) const {
    return VersionScratch{(uint64_t*)(p + pg), (uint32_t*)(p + next), (uint32_t*)(p + ja),
                          (uint32_t*)(p + jb), (uint32_t*)(p + mark), (uint64_t*)(p + sid),
                          (uint32_t*)(p + cnt), (uint32_t*)(p + forced), (uint64_t*)(p + part)};
  }
};

// The caller's runs as the kernels take them, and their total.
int runs_in(const lgs_run* runs, uint32_t nruns, MergeRun* out, uint32_t* n_total) {
  if (nruns > LGS_MERGE_MAX_RUNS)
    return fail(LGS_EINVAL, "%u runs: at most %d", nruns, LGS_MERGE_MAX_RUNS);
  if (nruns && !runs) return fail(LGS_EINVAL, "NULL argument");
  uint64_t n = 0;
  for (uint32_t r = 0; r < nruns; ++r) {
    const lgs_run& a = runs[r];
    if (a.n && (!a.keys || !a.key_off || !a.key_len || !a.vals || !a.val_off || !a.val_len))
      return fail(LGS_EINVAL, "NULL argument in run %u", r);
    out[r] = MergeRun{a.keys, a.key_off, a.key_len, a.vals, a.val_off, a.val_len, a.n, (uint32_t)n};
    n += a.n;
    if (n > kMaxEntries) return fail(LGS_EINVAL, "over 2^31 - 1 entries in all");
  }
  *n_total = (uint32_t)n;
  return LGS_OK;
}

int rule_in(int internal_keys, int drop, uint64_t smallest_snapshot, int drop_deletions,
            MergeRule* rule) {
  if ((internal_keys != 0 && internal_keys != 1) || (drop != 0 && drop != 1) ||
      (drop_deletions != 0 && drop_deletions != 1))
    return fail(LGS_EINVAL, "internal_keys, drop and drop_deletions must be 0 or 1");
  if (drop && !internal_keys) return fail(LGS_EINVAL, "drop needs internal_keys");
  *rule = MergeRule{(uint32_t)internal_keys, (uint32_t)drop, (uint32_t)(drop && drop_deletions),
                    smallest_snapshot};
  return LGS_OK;
}

}  // namespace

size_t lgs_merge_scratch(uint32_t n_total, uint32_t nruns) {
  if (n_total > kMaxEntries || nruns > LGS_MERGE_MAX_RUNS) return 0;
  return MergeLayout(n_total).total;
}

int lgs_merge_plan_dev(const lgs_run* runs, uint32_t nruns, int internal_keys, int drop,
                       uint64_t smallest_snapshot, int drop_deletions, uint64_t* d_counts,
                       void* d_scratch, size_t scratch_bytes, void* stream) {
  MergeRun in[kMergeMaxRuns];
  MergeRule rule;
  uint32_t n = 0;
  LGS_TRY(runs_in(runs, nruns, in, &n));
  LGS_TRY(rule_in(internal_keys, drop, smallest_snapshot, drop_deletions, &rule));
  if (!d_counts || !d_scratch) return fail(LGS_EINVAL, "NULL argument");
  const MergeLayout M(n);
  if (scratch_bytes < M.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_merge_scratch)", scratch_bytes, M.total);
  LGS_HIP(launch_merge_plan(in, nruns, n, rule, M.at((uint8_t*)d_scratch), d_counts,
                            (hipStream_t)stream));
  return LGS_OK;
}

size_t lgs_merge_version_scratch(uint32_t n_total, uint32_t nruns, uint64_t level_files,
                                 uint64_t level_key_bytes) {
  if (n_total > kMaxEntries || nruns > LGS_MERGE_MAX_RUNS || level_files > kMaxEntries ||
      level_key_bytes > (1ull << 40))
    return 0;
  return VersionLayout(n_total, level_files, level_key_bytes).total;
}

int lgs_merge_plan_version_dev(const lgs_run* runs, uint32_t nruns, uint64_t smallest_snapshot,
                               const lgs_level* levels, uint32_t nlevels,
                               uint64_t max_grandparent_overlap, uint64_t* d_counts,
                               void* d_scratch, size_t scratch_bytes, void* stream) {
  MergeRun in[kMergeMaxRuns];
  uint32_t n = 0;
  LGS_TRY(runs_in(runs, nruns, in, &n));
  if (nlevels > LGS_VERSION_MAX_LEVELS)
    return fail(LGS_EINVAL, "%u levels: at most %d", nlevels, LGS_VERSION_MAX_LEVELS);
  if (!d_counts || !d_scratch || (nlevels && !levels)) return fail(LGS_EINVAL, "NULL argument");
  uint64_t nfiles = 0, key_bytes = 0;
  for (uint32_t v = 0; v < nlevels; ++v) {
    if (levels[v].n > kMaxEntries) return fail(LGS_EINVAL, "level %u: over 2^31 - 1 files", v);
    if (levels[v].n && !levels[v].files) return fail(LGS_EINVAL, "NULL argument in level %u", v);
    for (uint32_t f = 0; f < levels[v].n; ++f) {
      const lgs_level_file& m = levels[v].files[f];
      if (!m.smallest || !m.largest) return fail(LGS_EINVAL, "NULL key in level %u", v);
      if (m.smallest_len < 8 || m.largest_len < 8)
        return fail(LGS_EINVAL, "level %u, file %u: an internal key under 8 bytes", v, f);
      key_bytes += (uint64_t)m.smallest_len + m.largest_len;
    }
    nfiles += levels[v].n;
  }
  if (nfiles > kMaxEntries || key_bytes > (1ull << 40))
    return fail(LGS_EINVAL, "%llu files in the levels", (unsigned long long)nfiles);
  const VersionLayout V(n, nfiles, key_bytes);
  if (scratch_bytes < V.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_merge_version_scratch)", scratch_bytes, V.total);
  // The levels in one upload: the files, level + 2's prefix sums, the keys.
  const uint32_t n0 = nlevels ? levels[0].n : 0;
  std::vector<uint8_t> up(V.up_end - V.files);
  VersionFile* files = (VersionFile*)up.data();
  uint64_t* P = (uint64_t*)(up.data() + (V.P - V.files));
  uint8_t* keys = up.data() + (V.keys - V.files);
  uint8_t* d = (uint8_t*)d_scratch;
  VersionDev dev{d + V.keys, (const VersionFile*)(d + V.files), (const uint64_t*)(d + V.P),
                 {0, 0, 0, 0, 0, 0}, nlevels, max_grandparent_overlap};
  uint64_t at = 0, f_at = 0;
  for (uint32_t v = 0; v < nlevels; ++v) {
    dev.first[v] = (uint32_t)f_at;
    for (uint32_t f = 0; f < levels[v].n; ++f, ++f_at) {
      const lgs_level_file& m = levels[v].files[f];
      files[f_at] = VersionFile{at, at + m.smallest_len, m.smallest_len, m.largest_len};
      memcpy(keys + at, m.smallest, m.smallest_len);
      memcpy(keys + at + m.smallest_len, m.largest, m.largest_len);
      at += (uint64_t)m.smallest_len + m.largest_len;
    }
  }
  for (uint32_t v = nlevels; v <= kVersionMaxLevels; ++v) dev.first[v] = (uint32_t)f_at;
  P[0] = 0;
  for (uint32_t f = 0; f < n0; ++f) {
    if (levels[0].files[f].file_size >= (1ull << 63) - P[f])
      return fail(LGS_EINVAL, "the files of level + 2 hold 2^63 bytes or more");
    P[f + 1] = P[f] + levels[0].files[f].file_size;
  }
  hipStream_t s = (hipStream_t)stream;
  // The upload reads `up`, so the stream is drained on every way out.
  const int rc = [&]() -> int {
    LGS_HIP(hipMemcpyAsync(d + V.files, up.data(), up.size(), hipMemcpyHostToDevice, s));
    const MergeRule rule{1, 1, 0, smallest_snapshot};
    LGS_HIP(launch_merge_plan_version(in, nruns, n, rule, V.M.at(d), dev, V.at(d), d_counts, s));
    return LGS_OK;
  }();
  const hipError_t drained = hipStreamSynchronize(s);
  LGS_TRY(rc);
  LGS_HIP(drained);
  return LGS_OK;
}

int lgs_merge_stops_dev(uint32_t n_total, uint32_t n_out, uint32_t* d_forced,
                        const void* d_scratch, size_t scratch_bytes, void* stream) {
  if (n_total > kMaxEntries || n_out > n_total)
    return fail(LGS_EINVAL, "%u entries out of %u", n_out, n_total);
  if (!d_scratch || (n_out && !d_forced)) return fail(LGS_EINVAL, "NULL argument");
  const VersionLayout V(n_total, 0, 0);
  if (scratch_bytes < V.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_merge_version_scratch)", scratch_bytes, V.total);
  if (n_out)
    LGS_HIP(hipMemcpyAsync(d_forced, (const uint8_t*)d_scratch + V.forced, 4 * (size_t)n_out,
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LGS_OK;
}

int lgs_merge_emit_dev(const lgs_run* runs, uint32_t nruns, uint32_t n_out, uint8_t* d_keys,
                       uint64_t* d_key_off, uint32_t* d_key_len, uint8_t* d_vals,
                       uint64_t* d_val_off, uint32_t* d_val_len, uint32_t* d_src_run,
                       uint32_t* d_src_index, void* d_scratch, size_t scratch_bytes,
                       void* stream) {
  MergeRun in[kMergeMaxRuns];
  uint32_t n = 0;
  LGS_TRY(runs_in(runs, nruns, in, &n));
  if (n_out > n) return fail(LGS_EINVAL, "%u entries out of %u", n_out, n);
  if (!d_key_off || !d_val_off || !d_scratch ||
      (n_out && (!d_keys || !d_key_len || !d_vals || !d_val_len || !d_src_run || !d_src_index)))
    return fail(LGS_EINVAL, "NULL argument");
  const MergeLayout M(n);
  if (scratch_bytes < M.total)
    return fail(LGS_EINVAL, "scratch %zu < %zu (lgs_merge_scratch)", scratch_bytes, M.total);
  LGS_HIP(launch_merge_emit(n, n_out, M.at((uint8_t*)d_scratch), d_keys, d_key_off,
                            d_key_len, d_vals, d_val_off, d_val_len, d_src_run, d_src_index,
                            (hipStream_t)stream));
  return LGS_OK;
}

int lgs_merge_host(const lgs_run* runs, uint32_t nruns, int internal_keys, int drop,
                   uint64_t smallest_snapshot, int drop_deletions, uint8_t* keys, size_t key_cap,
                   uint64_t* key_off, uint32_t* key_len, uint8_t* vals, size_t val_cap,
                   uint64_t* val_off, uint32_t* val_len, uint32_t* src_run, uint32_t* src_index,
                   uint32_t entry_cap, uint64_t* needed) {
  MergeRun in[kMergeMaxRuns];
  MergeRule rule;
  uint32_t n = 0;
  LGS_TRY(runs_in(runs, nruns, in, &n));
  LGS_TRY(rule_in(internal_keys, drop, smallest_snapshot, drop_deletions, &rule));
  if (!needed || !key_off || !val_off) return fail(LGS_EINVAL, "NULL argument");
  for (int k = 0; k < 5; ++k) needed[k] = 0;
  if (n == 0) {
    key_off[0] = val_off[0] = 0;
    return LGS_OK;
  }
  size_t kb = 0, vb = 0;
  for (uint32_t r = 0; r < nruns; ++r)
    for (uint32_t i = 0; i < in[r].n; ++i) {
      kb += in[r].key_len[i];
      vb += in[r].val_len[i];
    }
  Lease lease(batch_pool());
  LGS_TRY(lease.acquire());
  Ctx& c = lease.ctx();
  hipStream_t s = c.stream;
  const MergeLayout M(n);
  Layout L;  // uploads | downloads | device-only
  const size_t o_keys = L.take(kb + 16);
  const size_t o_vals = L.take(vb + 16);
  const size_t o_koff = L.take(8 * (size_t)n);
  const size_t o_voff = L.take(8 * (size_t)n);
  const size_t o_klen = L.take(4 * (size_t)n);
  const size_t o_vlen = L.take(4 * (size_t)n);
  const size_t up_end = L.at;
  const size_t o_cnt = L.take(8 * kMergeCounts);
  const size_t pin_end = L.at;
  const size_t o_scr = L.take(M.total);
  LGS_TRY(ctx_reserve(c, L.at, pin_end));
  uint8_t* h = c.h_buf;
  uint8_t* d = c.d_buf;
  {
    uint64_t* koff = (uint64_t*)(h + o_koff);
    uint64_t* voff = (uint64_t*)(h + o_voff);
    uint32_t* klen = (uint32_t*)(h + o_klen);
    uint32_t* vlen = (uint32_t*)(h + o_vlen);
    size_t ka = 0, va = 0;
    uint32_t e = 0;
    for (uint32_t r = 0; r < nruns; ++r) {
      const MergeRun& a = in[r];
      for (uint32_t i = 0; i < a.n; ++i, ++e) {
        koff[e] = ka;
        voff[e] = va;
        klen[e] = a.key_len[i];
        vlen[e] = a.val_len[i];
        memcpy(h + o_keys + ka, a.keys + a.key_off[i], a.key_len[i]);
        memcpy(h + o_vals + va, a.vals + a.val_off[i], a.val_len[i]);
        ka += a.key_len[i];
        va += a.val_len[i];
      }
    }
    memset(h + o_keys + kb, 0, 16);
    memset(h + o_vals + vb, 0, 16);
  }
  LGS_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, s));
  MergeRun dev[kMergeMaxRuns];
  for (uint32_t r = 0; r < nruns; ++r) {
    const size_t f = in[r].first;
    dev[r] = MergeRun{d + o_keys, (const uint64_t*)(d + o_koff) + f, (const uint32_t*)(d + o_klen) + f,
                      d + o_vals, (const uint64_t*)(d + o_voff) + f, (const uint32_t*)(d + o_vlen) + f,
                      in[r].n, in[r].first};
  }
  const MergeScratch w = M.at(d + o_scr);
  LGS_HIP(launch_merge_plan(dev, nruns, n, rule, w, (uint64_t*)(d + o_cnt), s));
  LGS_HIP(hipMemcpyAsync(h + o_cnt, d + o_cnt, 8 * kMergeCounts, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));   // the one read-back that sizes the outputs
  uint64_t cnt[kMergeCounts];
  memcpy(cnt, h + o_cnt, sizeof cnt);
  if (cnt[5] != ~0ull)
    return fail(LGS_EINVAL, "run %llu is not sorted%s", (unsigned long long)cnt[5],
                internal_keys ? " or has a key under 8 bytes" : "");
  for (int k = 0; k < 5; ++k) needed[k] = cnt[k];
  const uint64_t m = cnt[0], okb = cnt[1], ovb = cnt[2];
  if (m > n || okb > kb || ovb > vb)
    return fail(LGS_EINTERNAL, "%llu entries kept of %u", (unsigned long long)m, n);
  if (m > entry_cap || okb > key_cap || ovb > val_cap)
    return fail(LGS_ENOSPC,
                "%llu entries (entry_cap %u), keys %llu bytes (key_cap %zu), values %llu (val_cap %zu)",
                (unsigned long long)m, entry_cap, (unsigned long long)okb, key_cap,
                (unsigned long long)ovb, val_cap);
  if (!keys || !key_len || !vals || !val_len || !src_run || !src_index)
    return fail(LGS_EINVAL, "NULL argument");
  Layout O;
  const size_t q_keys = O.take((size_t)okb + 16);
  const size_t q_vals = O.take((size_t)ovb + 16);
  const size_t q_koff = O.take(8 * ((size_t)m + 1));
  const size_t q_voff = O.take(8 * ((size_t)m + 1));
  const size_t q_klen = O.take(4 * (size_t)m + 4);
  const size_t q_vlen = O.take(4 * (size_t)m + 4);
  const size_t q_run = O.take(4 * (size_t)m + 4);
  const size_t q_idx = O.take(4 * (size_t)m + 4);
  std::unique_ptr<Scratch> arena;
  LGS_TRY(scratch_alloc(&arena, O.at, s, "the merged entries"));
  uint8_t* e = (uint8_t*)arena->get();
  LGS_HIP(launch_merge_emit(n, (uint32_t)m, w, e + q_keys, (uint64_t*)(e + q_koff),
                            (uint32_t*)(e + q_klen), e + q_vals, (uint64_t*)(e + q_voff),
                            (uint32_t*)(e + q_vlen), (uint32_t*)(e + q_run),
                            (uint32_t*)(e + q_idx), s));
  // The uploads are no longer needed on the host: the downloads take their place.
  LGS_TRY(ctx_reserve(c, 0, O.at));
  h = c.h_buf;
  LGS_HIP(hipMemcpyAsync(h, e, O.at, hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  memcpy(keys, h + q_keys, (size_t)okb);
  memcpy(vals, h + q_vals, (size_t)ovb);
  memcpy(key_off, h + q_koff, 8 * ((size_t)m + 1));
  memcpy(val_off, h + q_voff, 8 * ((size_t)m + 1));
  memcpy(key_len, h + q_klen, 4 * (size_t)m);
  memcpy(val_len, h + q_vlen, 4 * (size_t)m);
  memcpy(src_run, h + q_run, 4 * (size_t)m);
  memcpy(src_index, h + q_idx, 4 * (size_t)m);
  return LGS_OK;
}
