/*
 * lcdb_gpu_snappy.h -- C ABI of the MI355X (gfx950) Snappy block codec.
 *
 * Two layers, both plain C (C89-compatible declarations, no HIP or torch
 * types; streams are passed as `void *` holding a hipStream_t):
 *
 * 1. The drop-in.  The four symbols lcdb's codec exports, with identical
 *    names, argument meaning and return values, so lcdb's src/table/ (*.c) and
 *    src/builder.c link against this library unchanged in place of
 *    src/util/snappy.c (CMakeLists.txt:209 / Makefile.am:86-87):
 *
 *      ldb_snappy_encode_size  replaces  src/util/snappy.c:347-362
 *                                        (declared snappy.h:28-29)
 *      ldb_snappy_encode       replaces  src/util/snappy.c:364-384
 *                                        (declared snappy.h:31-32)
 *      ldb_snappy_decode_size  replaces  src/util/snappy.c:386-399
 *                                        (declared snappy.h:34-35)
 *      ldb_snappy_decode       replaces  src/util/snappy.c:401-412
 *                                        (declared snappy.h:37-38)
 *
 *    Callers: src/table/table_builder.c:182,187 (encode) and
 *    src/table/format.c:237,247 (decode); both pass pageable host buffers.
 *    Both are thread-safe.  A call leases one of a bounded pool of staging
 *    slots (per device: at most LGS_DROPIN_SLOTS = 8 slots of LGS_DROPIN_MB =
 *    4 MiB pinned + 4 MiB device memory, created on first use; a caller waits
 *    while all are leased), so the drop-in's memory is bounded whatever the
 *    input: encode runs any input through its slot in passes of whole 64 KiB
 *    chunks (independent, snappy.c:370-381); decode rejects on the host every
 *    stream whose size header its length cannot satisfy (exactly the
 *    reference's result, no device work), and decodes a block larger than a
 *    slot in device memory taken for that call only.
 *    Compressed bytes are identical to the reference encoder's and decode
 *    accepts/rejects exactly what the reference does.  The *_size functions
 *    are header arithmetic (a bound, a varint32 read) and run on the host.
 *    Errors: lcdb's encode path has no error return (table_builder.c:182-
 *    188), so ldb_snappy_encode aborts with a diagnostic only when the device
 *    fails (or no slot at all can be created); ldb_snappy_decode returns 0
 *    (LDB_CORRUPTION at format.c:247-251) with a diagnostic when device
 *    memory for an over-slot block runs out, and aborts only when the device
 *    fails.  There is no CPU fallback.  On a decode failure the contents of
 *    zp are unspecified, as in the reference.
 *
 * 2. The batched API (lgs_*), new: tens of thousands of independent blocks
 *    per launch.  Blocks are addressed by byte offsets into one base buffer.
 *    Output per block is byte-identical to ldb_snappy_encode on that block
 *    alone (encode) / to ldb_snappy_decode (decode).
 *
 *    Return values: LGS_OK (0) or a negative LGS_E* code; lgs_last_error()
 *    gives a message for the calling thread.
 */
#ifndef LCDB_GPU_SNAPPY_H
#define LCDB_GPU_SNAPPY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- drop-in: src/util/snappy.h:28-38 ---- */
int ldb_snappy_encode_size(size_t *zn, size_t xn);
size_t ldb_snappy_encode(uint8_t *zp, const uint8_t *xp, size_t xn);
int ldb_snappy_decode_size(size_t *zn, const uint8_t *xp, size_t xn);
int ldb_snappy_decode(uint8_t *zp, const uint8_t *xp, size_t xn);

/* ---- batched API ---- */
#define LGS_OK          0
#define LGS_EINVAL     -1   /* bad argument (NULL, size out of range)   */
#define LGS_EHIP       -2   /* HIP runtime error                        */
#define LGS_ENODEV     -3   /* no usable gfx950 device                  */
#define LGS_ENOMEM     -4   /* device / pinned allocation failed        */
#define LGS_ENOSPC     -5   /* output buffer too small                  */
#define LGS_EINTERNAL  -6   /* a device result broke its own bound      */

/* Per-block decode status written by the decode calls. */
#define LGS_ST_CORRUPT  0   /* reference decode would return 0          */
#define LGS_ST_OK       1
#define LGS_ST_NOSPACE  2   /* decoded length > out_cap[i]              */

/* Worst-case encoded size (same formula as ldb_snappy_encode_size). */
size_t lgs_encode_bound(size_t n);

/* Device-resident encode.  All pointers are device pointers.  Block i is
   d_in[d_in_off[i] .. + d_in_len[i]) (any length < 2^31; blocks over
   64 KiB are encoded as consecutive 64 KiB chunks by one wave, exactly as
   snappy.c:370-381 does); its encoding is written at d_out + d_out_off[i]
   (room for lgs_encode_bound(d_in_len[i]) bytes) and its length to
   d_out_len[i].  max_in_len >= every d_in_len[i] (selects the LDS class).  Asynchronous on
   `stream` (a hipStream_t, NULL = default stream). */
int lgs_encode_batch_dev(const uint8_t *d_in, const uint64_t *d_in_off,
                         const uint32_t *d_in_len, uint8_t *d_out,
                         const uint64_t *d_out_off, uint32_t *d_out_len,
                         uint32_t n, uint32_t max_in_len, void *stream);

/* Device-resident decode.  Block i is d_in[d_in_off[i] .. + d_in_len[i]);
   it decodes into d_out + d_out_off[i] (capacity d_out_cap[i]);
   d_out_len[i] = decoded length (0 unless ok), d_status[i] = LGS_ST_*.
   max_out_cap >= every d_out_cap[i].  Asynchronous on `stream`.
   Read slack: the kernel may READ (never write) up to 16 bytes past the end
   of a block's input and past its output cursor, so both allocations must
   extend at least 16 bytes beyond the last block.
   Both _dev calls: a batch of >= 512 blocks whose largest block is over
   4 608 bytes is sorted into size classes on the device first, with up to
   16 bytes per block of stream-ordered scratch from a private memory pool
   of the device (hipMallocFromPoolAsync, freed on `stream`; the process's
   default pool is not touched); LGS_ENOMEM-class HIP errors are possible
   there.  lgs_set_option("split", "0") turns this off. */
int lgs_decode_batch_dev(const uint8_t *d_in, const uint64_t *d_in_off,
                         const uint32_t *d_in_len, uint8_t *d_out,
                         const uint64_t *d_out_off, const uint32_t *d_out_cap,
                         uint32_t *d_out_len, uint8_t *d_status, uint32_t n,
                         uint32_t max_out_cap, void *stream);

/* Host-buffer variants: same layout with host pointers (pageable is fine).
   Data moves through pinned staging with hipMemcpyAsync on a pooled
   context's stream (contexts are leased per call, never tied to a thread;
   their arenas grow to the largest batch served); the call returns when the
   results are in the caller's buffers. */
int lgs_encode_batch_host(const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, uint8_t *out,
                          const uint64_t *out_off, uint32_t *out_len,
                          uint32_t n);
int lgs_decode_batch_host(const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, uint8_t *out,
                          const uint64_t *out_off, const uint32_t *out_cap,
                          uint32_t *out_len, uint8_t *status, uint32_t n);

/* ---- SSTable block framing ----
 *
 * lcdb frames every table block as  contents | type (1 byte) | masked
 * crc32c of contents+type (fixed32)  (table_builder.c:123-153), and reads a
 * block back through format.c:162-270.  These calls do both for many blocks
 * per launch, byte-identical to the reference doing them one at a time. */

#define LGS_NO_COMPRESSION      0   /* enum ldb_compression (options.h)       */
#define LGS_SNAPPY_COMPRESSION  1
#define LGS_TRAILER_SIZE        5   /* LDB_TRAILER_SIZE (format.h:34)         */

/* Further per-block read statuses (besides LGS_ST_CORRUPT/OK/NOSPACE). */
#define LGS_ST_IOERR    3   /* truncated block read -> LDB_IOERR (format.c:195-198)     */
#define LGS_ST_BADCRC   4   /* checksum mismatch -> LDB_CORRUPTION (format.c:203-211)   */
#define LGS_ST_BADTYPE  5   /* bad block type -> LDB_CORRUPTION (format.c:263-267)      */

/* Row 1.  d_crc[i] = ldb_crc32c_value(block i) (crc32c.c:1147, crc32c.h:29),
   extended over the byte d_type[i] when d_type != NULL (table_builder.c:139-
   140), then ldb_crc32c_mask'ed (crc32c.h:46-50) when masked != 0.  With a
   type and masked = 1 this is the trailer's crc field.  Asynchronous. */
int lgs_crc32c_batch_dev(const uint8_t *d_in, const uint64_t *d_in_off,
                         const uint32_t *d_in_len, const uint8_t *d_type,
                         int masked, uint32_t *d_crc, uint32_t n, void *stream);

/* Row 2.  n finished data blocks (ldb_blockgen_finish output, raw bytes)
   written as ldb_tablegen_write_block writes them (table_builder.c:155-213):
   snappy-encoded when compression = LGS_SNAPPY_COMPRESSION and that saves
   more than 12.5 % (:190), else raw; each followed by its trailer; block i at
   file offset handle_off[i] with handle_size[i] content bytes (:128-129);
   the first block at offset `base`.  d_file[j] receives file offset base + j;
   *d_end = base + bytes written.  d_file needs sum(raw_len) + 5n bytes.
   raw_total = sum of the raw lengths (sizes the scratch);
   d_scratch: lgs_table_write_scratch(n, raw_total) device bytes.  Inputs
   must stay readable 16 bytes past each block.  Asynchronous. */
size_t lgs_table_write_scratch(uint32_t n, uint64_t raw_total);
int lgs_table_write_dev(const uint8_t *d_raw, const uint64_t *d_raw_off,
                        const uint32_t *d_raw_len, uint32_t n, uint32_t max_raw_len,
                        uint64_t raw_total, int compression, uint64_t base,
                        uint8_t *d_file, uint64_t *d_handle_off,
                        uint64_t *d_handle_size, uint64_t *d_end,
                        void *d_scratch, size_t scratch_bytes, void *stream);
/* Host buffers; returns when file/handles/end are written.  file_cap: room
   in `file` (sum(raw_len) + 5n always suffices). */
int lgs_table_write_host(const uint8_t *raw, const uint64_t *raw_off,
                         const uint32_t *raw_len, uint32_t n, int compression,
                         uint64_t base, uint8_t *file, size_t file_cap,
                         uint64_t *handle_off, uint64_t *handle_size,
                         uint64_t *end);

/* Row 3.  ldb_read_block (format.c:162-270) for n block handles of one
   table image (d_file[0 .. file_len) = file offsets 0 ..): truncation check,
   trailer check when verify_checksums, then raw copy or snappy decode into
   d_out + d_out_off[i] (capacity d_out_cap[i]; the decoded size of a snappy
   block is its varint32 header, ldb_snappy_decode_size).  d_status[i] =
   LGS_ST_OK or the reason the reference fails; d_out_len[i] = contents
   length when ok (the output bytes of a block that fails are unspecified).
   With verify_checksums the CRC checks run on a second stream of the
   library's own beside the decoder (lgs_set_option("verify_overlap", "0")
   or LGS_VERIFY_OVERLAP=0: inside the type dispatch); the call stays
   ordered on `stream`.  d_file must stay readable 16 bytes past file_len.
   d_scratch: lgs_table_read_scratch(n) device bytes.  Asynchronous. */
size_t lgs_table_read_scratch(uint32_t n);
int lgs_table_read_dev(const uint8_t *d_file, uint64_t file_len,
                       const uint64_t *d_handle_off, const uint64_t *d_handle_size,
                       uint32_t n, int verify_checksums, uint8_t *d_out,
                       const uint64_t *d_out_off, const uint32_t *d_out_cap,
                       uint32_t max_out_cap, uint32_t *d_out_len, uint8_t *d_status,
                       void *d_scratch, size_t scratch_bytes, void *stream);
/* Host buffers (e.g. an mmap'd .ldb); only the handles' byte ranges are
   uploaded.  Returns when out/out_len/status are written. */
int lgs_table_read_host(const uint8_t *file, uint64_t file_len,
                        const uint64_t *handle_off, const uint64_t *handle_size,
                        uint32_t n, int verify_checksums, uint8_t *out,
                        const uint64_t *out_off, const uint32_t *out_cap,
                        uint32_t *out_len, uint8_t *status);

/* Row 3, opening a table: ldb_table_open (table.c:120-180) and the index
   walk of its two-level iterator, for the batched read above.  From the
   footer (format.c:116-137) it reads the index block through
   lgs_table_read_host (checksums verified when paranoid_checks, as
   table.c:148-151) and returns, in index order, each entry's data-block
   handle (handle_off/handle_size, cap of them; *count written) and, if keys
   != NULL, its separator key (keys[key_off[i] .. key_off[i+1]), keys_cap
   bytes, key_off has cap + 1 entries).  internal_keys: index keys are
   internal keys (the DB's tables), so one under 8 bytes is a bad entry
   (block.c:270-273).  With filter_name (e.g.
   "filter.leveldb.BuiltinBloomFilter2") the metaindex is read too and
   *filter_off and *filter_size receive that entry's handle, or ~0 / 0 when
   there is none or the metaindex does not read (table.c:78-120 ignores
   those errors).  *status: LGS_ST_OK; LGS_ST_CORRUPT for a short file, a
   bad footer, a bad index block or entry (the walk stops there), or an
   entry whose value is no handle (skipped, as the two-level iterator skips
   it); the block read's own status (LGS_ST_IOERR, _BADCRC, _BADTYPE) when
   the index block does not read.  Returns LGS_ENOSPC when cap or keys_cap is
   too small. */
int lgs_table_index_host(const uint8_t *file, uint64_t file_len, int paranoid_checks,
                         int internal_keys, const char *filter_name, uint64_t *handle_off,
                         uint64_t *handle_size, uint32_t cap, uint32_t *count, uint8_t *keys,
                         size_t keys_cap, uint64_t *key_off, uint64_t *filter_off,
                         uint64_t *filter_size, uint8_t *status);

/* Row 4.  lcdb's builtin bloom filter (src/util/bloom.c, src/util/hash.c):
   filter f holds keys [first[f], first[f+1]) and is written at out +
   out_off[f] exactly as ldb_bloom_build appends it (bloom.c:102-119):
   lgs_bloom_filter_size(n, bits_per_key) bytes = the bit array
   (max(64, n * bits_per_key) bits, rounded up to bytes) + one byte k
   (bits_per_key * 0.69, clamped to [1, 30]); an empty filter has no bytes
   (filter_block.c:89-93).  match[q] = ldb_bloom_match(filter
   query_filter[q], key q) (bloom.c:121-165).  Keys must stay readable 16
   bytes past their end.  The _dev calls are asynchronous. */
size_t lgs_bloom_filter_size(uint32_t nkeys, int bits_per_key);
int lgs_bloom_build_dev(const uint8_t *d_keys, const uint64_t *d_key_off,
                        const uint32_t *d_key_len, const uint32_t *d_first,
                        uint32_t nfilters, int bits_per_key, uint8_t *d_out,
                        const uint64_t *d_out_off, void *stream);
int lgs_bloom_match_dev(const uint8_t *d_filters, const uint64_t *d_filter_off,
                        const uint32_t *d_filter_len, const uint32_t *d_query_filter,
                        const uint8_t *d_keys, const uint64_t *d_key_off,
                        const uint32_t *d_key_len, uint8_t *d_match, uint32_t nq,
                        void *stream);
int lgs_bloom_build_host(const uint8_t *keys, const uint64_t *key_off,
                         const uint32_t *key_len, const uint32_t *first,
                         uint32_t nfilters, int bits_per_key, uint8_t *out,
                         const uint64_t *out_off);
int lgs_bloom_match_host(const uint8_t *filters, const uint64_t *filter_off,
                         const uint32_t *filter_len, uint32_t nfilters,
                         const uint32_t *query_filter, const uint8_t *keys,
                         const uint64_t *key_off, const uint32_t *key_len, uint32_t nq,
                         uint8_t *match);

/* Row 4, the filter block of one table (src/table/filter_block.c), as
   lcdb's table builder makes it: data block b holds keys [block_first[b],
   block_first[b+1]) and sits at file offset block_off[b] (file order, the
   first at 0); data_end is the offset after the last one.  The builder adds
   each block's keys, writes the block, then calls
   ldb_filtergen_start_block(offset after it) (table_builder.c:242-243,
   276-277) and ldb_filtergen_finish at the end (:294): one bloom filter per
   started 2 KiB of data offsets (filter_block.c:79-121), then the u32
   offset array, its start and base_lg = 11 (:131-150).  internal_keys = 1
   is the DB's internal filter policy (dbformat.c:308-334): keys are internal
   keys and filters cover the user key, i.e. all but the last 8 bytes.
   Keys must stay readable 16 bytes past their end; block_first and
   block_off must not decrease, block_off[nblocks-1] <= data_end (checked by
   _host; the _dev caller's contract, as for handles from lgs_table_write_dev).
   Sizes: lgs_filter_block_bound(...) bytes of out suffice;
   lgs_filter_block_scratch(data_end) bytes of device scratch for _dev, whose
   block length lands in *d_size.  The _dev calls are asynchronous. */
size_t lgs_filter_block_bound(uint32_t nkeys, uint32_t nblocks, uint64_t data_end,
                              int bits_per_key);
size_t lgs_filter_block_scratch(uint64_t data_end);
int lgs_filter_block_build_dev(const uint8_t *d_keys, const uint64_t *d_key_off,
                               const uint32_t *d_key_len, uint32_t nkeys,
                               const uint32_t *d_block_first, const uint64_t *d_block_off,
                               uint32_t nblocks, uint64_t data_end, int bits_per_key,
                               int internal_keys, uint8_t *d_out, size_t out_cap,
                               uint64_t *d_size, void *d_scratch, size_t scratch_bytes,
                               void *stream);
int lgs_filter_block_build_host(const uint8_t *keys, const uint64_t *key_off,
                                const uint32_t *key_len, const uint32_t *block_first,
                                const uint64_t *block_off, uint32_t nblocks, uint64_t data_end,
                                int bits_per_key, int internal_keys, uint8_t *out,
                                size_t out_cap, size_t *size);
/* ldb_filter_matches (filter_block.c:170-225) of the filter block
   block[0 .. block_len) -- as ldb_filter_init parses it -- for query q =
   (key q, the data block at file offset block_offset[q]): 0 = the key is
   certainly absent from that block, 1 = it may be present (also for every
   malformed filter block or offset out of its range). */
int lgs_filter_block_match_dev(const uint8_t *d_block, size_t block_len,
                               const uint64_t *d_block_offset, const uint8_t *d_keys,
                               const uint64_t *d_key_off, const uint32_t *d_key_len, uint32_t nq,
                               int internal_keys, uint8_t *d_match, void *stream);
int lgs_filter_block_match_host(const uint8_t *block, size_t block_len,
                                const uint64_t *block_offset, const uint8_t *keys,
                                const uint64_t *key_off, const uint32_t *key_len, uint32_t nq,
                                int internal_keys, uint8_t *match);

/* ---- building tables from sorted entries ----
 *
 * The data blocks lcdb's table builder makes from n entries in key order:
 * ldb_tablegen_add (table_builder.c:215-255) appends each entry with
 * ldb_blockgen_add (block_builder.c:91-136: shared | non_shared | value_size
 * varint32s, the key's unshared bytes, the value; shared = 0 at every
 * restart_interval-th entry of a block), and flushes the block through
 * ldb_blockgen_finish (:138-151: the restart offsets and their count) as soon
 * as ldb_blockgen_size_estimate (:153-158) reaches block_size
 * (table_builder.c:251-254).  Entry i has key d_keys[d_key_off[i] ..
 * + d_key_len[i]) and value d_vals[d_val_off[i] .. + d_val_len[i]); both
 * buffers must stay readable 16 bytes past their end.
 *
 * Results: block b holds entries [d_block_first[b], d_block_first[b+1]) and
 * is the d_raw_len[b] bytes at d_raw + d_raw_off[b], blocks packed one after
 * the other -- the input lgs_table_write_dev takes; its index key (what the
 * builder adds to the index block, table_builder.c:229-239, 332-341) is
 * d_ikey[d_ikey_off[b] .. d_ikey_off[b+1]): the comparator's shortest
 * separator of block b's last key and block b+1's first, its short successor
 * of the last key for the last block.  internal_keys = 0: lcdb's bytewise
 * comparator (comparator.c:44-88); 1: the DB's internal-key comparator
 * (dbformat.c:232-285), which shortens the user key (all but the last 8
 * bytes) and appends the fixed64 pack_seqtype(LDB_MAX_SEQUENCE,
 * LDB_VALTYPE_SEEK) only when that user key got physically shorter.
 *
 * Limits: n < 2^31; every key + value under 2^30 bytes; every finished block
 * under 2^31; restart_interval >= 1; with internal_keys every key has at
 * least 8 bytes; keys strictly increase under the comparator, as lcdb
 * asserts (block_builder.c:102-103) -- not checked.  The _host calls check
 * the others (LGS_EINVAL) before any device work; they are the _dev caller's
 * contract.  n = 0 yields no block.
 *
 * Two device calls, because the host needs the block count between them to
 * size what follows.  lgs_block_cut_dev finds the blocks: it writes
 * d_block_first, d_raw_off and d_ikey_off (room for n + 1 values each; entry
 * [blocks] of the offsets is the total), d_raw_len (n) and d_counts[4] =
 * {blocks, bytes of all raw blocks, longest block, bytes of all index keys}.
 * lgs_block_emit_dev then writes the blocks into d_raw (d_counts[1] + 16
 * bytes; lgs_block_build_bound(n, key bytes, value bytes) always suffices)
 * and, unless d_ikey is NULL, the index keys into d_ikey (d_counts[3] bytes,
 * at most the keys' total).  Both take the same lgs_block_build_scratch(n)
 * bytes of device scratch, which must be left alone between them, and both
 * are asynchronous on `stream`. */
size_t lgs_block_build_bound(uint32_t n, uint64_t key_bytes, uint64_t value_bytes);
size_t lgs_block_build_scratch(uint32_t n);
int lgs_block_cut_dev(const uint8_t *d_keys, const uint64_t *d_key_off,
                      const uint32_t *d_key_len, const uint32_t *d_val_len, uint32_t n,
                      uint64_t block_size, uint32_t restart_interval, int internal_keys,
                      uint32_t *d_block_first, uint64_t *d_raw_off, uint32_t *d_raw_len,
                      uint64_t *d_ikey_off, uint64_t *d_counts, void *d_scratch,
                      size_t scratch_bytes, void *stream);
int lgs_block_emit_dev(const uint8_t *d_keys, const uint64_t *d_key_off,
                       const uint32_t *d_key_len, const uint8_t *d_vals,
                       const uint64_t *d_val_off, const uint32_t *d_val_len, uint32_t n,
                       uint32_t restart_interval, int internal_keys, uint32_t nblocks,
                       const uint32_t *d_block_first, const uint64_t *d_raw_off,
                       const uint32_t *d_raw_len, uint8_t *d_raw, const uint64_t *d_ikey_off,
                       uint8_t *d_ikey, void *d_scratch, size_t scratch_bytes, void *stream);
/* Host arrays in and out (a pooled context, one synchronisation between cut
   and emit).  raw_off, block_first and ikey_off need n + 1 entries, raw_len
   n; LGS_ENOSPC when raw_cap or ikey_cap is too small. */
int lgs_block_build_host(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                         const uint8_t *vals, const uint64_t *val_off, const uint32_t *val_len,
                         uint32_t n, uint64_t block_size, uint32_t restart_interval,
                         int internal_keys, uint8_t *raw, size_t raw_cap, uint64_t *raw_off,
                         uint32_t *raw_len, uint32_t *block_first, uint8_t *ikey,
                         size_t ikey_cap, uint64_t *ikey_off, uint32_t *nblocks);

/* The whole .ldb that ldb_tablegen_add for every entry and ldb_tablegen_finish
   write (table_builder.c:215-365), byte for byte: the data blocks above
   framed as lgs_table_write_dev frames them; with bits_per_key > 0 the filter
   block of lgs_filter_block_build_dev, stored raw (:292-299); the metaindex
   block (:301-328: the entry "filter.leveldb.BuiltinBloomFilter2" -> the
   filter's handle, or no entry); the index block (:330-344: index key ->
   ldb_handle_export of the block's handle, restart interval 1, :87), built by
   the block builder itself; the 48-byte footer (format.c:92-106).  Everything
   that grows with the table stays on the device until the one download of
   the image; metaindex and footer are assembled on the host.  No entries
   gives lcdb's empty table.  file_cap: lgs_table_build_bound(...) always
   suffices; LGS_ENOSPC (with *file_size set when it is known) otherwise. */
size_t lgs_table_build_bound(uint32_t n, uint64_t key_bytes, uint64_t value_bytes,
                             int bits_per_key);
int lgs_table_build_host(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                         const uint8_t *vals, const uint64_t *val_off, const uint32_t *val_len,
                         uint32_t n, uint64_t block_size, uint32_t restart_interval,
                         int compression, int bits_per_key, int internal_keys, uint8_t *file,
                         size_t file_cap, size_t *file_size);

/* The same build with the entries in device memory and the images left there,
   cut into the files a compaction writes (db_impl.c:1399-1425): after every
   ldb_tablegen_add the output file is closed once ldb_tablegen_size reaches
   max_file_size.  That size moves only when a block is flushed
   (table_builder.c:251-254, :384-386), so a file ends directly after a block
   flush: the files' data blocks are the blocks of one continuous cut over all
   entries, a file that starts at block s ends after the first block whose
   framed end lies max_file_size or more past the start of s, and per file
   only the handle offsets (from the file's start), the index key of the last
   block (the comparator's short successor, :332-341), the filter block, the
   metaindex, the index block and the footer are the file's own.
   max_file_size = UINT64_MAX gives one file, the image of
   lgs_table_build_host; max_file_size = 0 would close a file after every
   entry with a block pending, which is no block boundary: LGS_EINVAL.

   Entries: the layout lgs_merge_emit_dev and lgs_block_entries_emit_dev write
   (lgs_block_cut_dev's limits and contract); key_bytes and value_bytes are
   the totals of the keys and values.  File f is the d_file_size[f] bytes at
   d_files + d_file_off[f] (starts 16-aligned, the images complete .ldb files
   byte for byte as lcdb writes them) and holds entries [d_file_first[f],
   d_file_first[f + 1]).  d_file_off and d_file_size have files_cap_count
   entries, d_file_first files_cap_count + 1; *n_files and *files_bytes (the
   end of the last image's room in d_files) are host outputs.
   lgs_tables_build_bound(...) always suffices for files_cap and sets
   *max_files to a files_cap_count that does.  LGS_ENOSPC when files_cap or
   files_cap_count is too small, with *n_files and *files_bytes set to what
   this call needs and nothing written to the d_file arrays.  n = 0 gives no
   file (*n_files = 0, LGS_OK): compaction opens no output without a kept
   entry; this differs on purpose from lgs_table_build_host, whose n = 0 is
   lcdb's empty table.  Other bad arguments as lgs_table_build_host.

   Scratch comes from a pooled context.  The call synchronises `stream` (for
   the block count, the file count, one row of counts per file, and once per
   file for its index and filter block sizes) and has drained it when it
   returns; no entry, block or image byte crosses the link, only those counts
   and each file's host-assembled metaindex block. */
size_t lgs_tables_build_bound(uint32_t n, uint64_t key_bytes, uint64_t value_bytes,
                              int bits_per_key, uint64_t max_file_size, uint32_t *max_files);
int lgs_tables_build_dev(const uint8_t *d_keys, const uint64_t *d_key_off,
                         const uint32_t *d_key_len, const uint8_t *d_vals,
                         const uint64_t *d_val_off, const uint32_t *d_val_len, uint32_t n,
                         uint64_t key_bytes, uint64_t value_bytes, uint64_t block_size,
                         uint32_t restart_interval, int compression, int bits_per_key,
                         int internal_keys, uint64_t max_file_size, uint8_t *d_files,
                         size_t files_cap, uint64_t *d_file_off, uint64_t *d_file_size,
                         uint32_t *d_file_first, uint32_t files_cap_count, uint32_t *n_files,
                         uint64_t *files_bytes, void *stream);

/* The cut and the build with forced starts: a compaction closes
   its output file before a key when ldb_compaction_should_stop_before says so
   (db_impl.c:1354-1360), and ldb_finish_compaction_output_file flushes the
   pending block, so such a file start is a block start that the size rule did
   not choose.  d_forced: n uint32 flags in device memory as
   lgs_merge_stops_dev writes them, or NULL; entry i > 0 with a nonzero flag
   starts a block and a file (flag 0 is ignored: entry 0 starts both anyway).
   The block that starts at s ends at the size rule's place or before the
   first forced start behind s, whichever comes first; a file that starts at
   block s ends after the first block that reaches max_file_size or before
   the next block whose first entry is forced.  Everything else is
   lgs_block_cut_dev and lgs_tables_build_dev, which are the NULL case of
   these calls.  lgs_tables_build_forced_bound counts n_forced (the number of
   nonzero flags, lgs_merge_plan_version_dev's d_counts[6]) more files. */
int lgs_block_cut_forced_dev(const uint8_t *d_keys, const uint64_t *d_key_off,
                             const uint32_t *d_key_len, const uint32_t *d_val_len, uint32_t n,
                             uint64_t block_size, uint32_t restart_interval, int internal_keys,
                             const uint32_t *d_forced, uint32_t *d_block_first,
                             uint64_t *d_raw_off, uint32_t *d_raw_len, uint64_t *d_ikey_off,
                             uint64_t *d_counts, void *d_scratch, size_t scratch_bytes,
                             void *stream);
size_t lgs_tables_build_forced_bound(uint32_t n, uint64_t key_bytes, uint64_t value_bytes,
                                     int bits_per_key, uint64_t max_file_size, uint32_t n_forced,
                                     uint32_t *max_files);
int lgs_tables_build_forced_dev(const uint8_t *d_keys, const uint64_t *d_key_off,
                                const uint32_t *d_key_len, const uint8_t *d_vals,
                                const uint64_t *d_val_off, const uint32_t *d_val_len, uint32_t n,
                                uint64_t key_bytes, uint64_t value_bytes, uint64_t block_size,
                                uint32_t restart_interval, int compression, int bits_per_key,
                                int internal_keys, uint64_t max_file_size,
                                const uint32_t *d_forced, uint8_t *d_files, size_t files_cap,
                                uint64_t *d_file_off, uint64_t *d_file_size,
                                uint32_t *d_file_first, uint32_t files_cap_count,
                                uint32_t *n_files, uint64_t *files_bytes, void *stream);

/* ---- batched point lookups ----
 *
 * ldb_blockiter_create + one ldb_blockiter_seek on the fresh iterator
 * (block.c:324-451) for nq independent queries.  Query q seeks key
 * d_keys[d_key_off[q] .. + d_key_len[q]) in block d_query_block[q]; block b =
 * d_blocks[d_block_off[b] .. + d_block_len[b]), a decoded block as
 * lgs_table_read_dev leaves it.  A query block index >= nblocks (0xffffffff
 * by convention) names no block: no entry, LGS_ST_OK.  d_block_status may be
 * NULL, else a block whose status != LGS_ST_OK yields that status and no
 * entry (an error iterator, table.c:286-297).  internal_keys = 0: lcdb's
 * bytewise comparator; 1: ldb_ikc_compare (dbformat.c:206-230), and a target
 * or stored key under 8 bytes is corrupt as block.c has it.  No other
 * comparator is supported.  The outcome is the reference's for any block
 * contents, sorted or not; nothing outside a block's bytes and a key's bytes
 * is read.
 *
 * Outputs per query: d_entry_pos (offset of the found entry in its block,
 * 0xffffffff = no entry), d_found_key_len, d_val_pos / d_val_len (the value,
 * an offset into the block), d_status (LGS_ST_OK, LGS_ST_CORRUPT or the
 * block's status); if d_key_out != NULL the found entry's full key, its first
 * min(length, d_key_out_cap[q]) bytes at d_key_out + d_key_out_off[q].
 * d_scratch: lgs_block_seek_scratch(nq) device bytes.  Asynchronous. */
size_t lgs_block_seek_scratch(uint32_t nq);
int lgs_block_seek_dev(const uint8_t *d_blocks, const uint64_t *d_block_off,
                       const uint32_t *d_block_len, const uint8_t *d_block_status,
                       uint32_t nblocks, const uint32_t *d_query_block, const uint8_t *d_keys,
                       const uint64_t *d_key_off, const uint32_t *d_key_len, uint32_t nq,
                       int internal_keys, uint32_t *d_entry_pos, uint32_t *d_found_key_len,
                       uint32_t *d_val_pos, uint32_t *d_val_len, uint8_t *d_status,
                       uint8_t *d_key_out, const uint64_t *d_key_out_off,
                       const uint32_t *d_key_out_cap, void *d_scratch, size_t scratch_bytes,
                       void *stream);

/* What version_set.c's save_value (:373-388) leaves in its saver. */
#define LGS_GET_NOTFOUND  0
#define LGS_GET_FOUND     1
#define LGS_GET_DELETED   2
#define LGS_GET_CORRUPT   3

/* ldb_table_internal_get (table.c:314-364) for nq keys against one table
   image (file[0 .. file_len), e.g. an mmap'd .ldb), opened as ldb_table_open
   opens it (paranoid_checks: the index and filter blocks' checksums;
   filter_name as for lgs_table_index_host, NULL = no filter policy).  Key q =
   keys[key_off[q] .. + key_len[q]).  Per query: called[q] = 1 when
   handle_result would be called, then its key and value are
   out[out_key_off[q] .. out_val_off[q]) and out[out_val_off[q] ..
   out_key_off[q + 1]) (nq + 1 offsets each, results packed in query order);
   status[q] = the LGS_ST_* of the rc the reference returns (LGS_ST_OK,
   LGS_ST_CORRUPT, or a block read's LGS_ST_IOERR / _BADCRC / _BADTYPE).  A
   table that does not open (short file, bad footer, unreadable index block)
   gives every query that status and no result.  verdict (may be NULL; with
   internal_keys = 1): LGS_GET_* for the found entry against key q's user
   key; LGS_GET_NOTFOUND where nothing was found.
   Returns LGS_ENOSPC with *out_needed = the bytes the results take when
   out_cap is smaller (called and status are written then, out is not);
   LGS_EINVAL for NULL or inconsistent arguments before any device work.
   The index block is read and searched on the device; the handles it yields
   come back to the host once to size the read of the distinct data blocks. */
int lgs_table_get_host(const uint8_t *file, uint64_t file_len, int verify_checksums,
                       int paranoid_checks, int internal_keys, const char *filter_name,
                       const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                       uint32_t nq, uint8_t *called, uint8_t *status, uint8_t *verdict,
                       uint8_t *out, size_t out_cap, uint64_t *out_key_off,
                       uint64_t *out_val_off, size_t *out_needed);

/* ---- opened tables ----
 *
 * lgs_table_get_host opens the table on every call: it reads and decodes the
 * index and filter blocks each time.  An opened table does that once, as
 * ldb_table_open (table.c:120-180) does, and keeps on the device the decoded
 * index block, its length and status, and the decoded filter block; gets then
 * run against them as ldb_table_internal_get runs against an ldb_table_t.
 *
 * lgs_table_open_host: paranoid_checks, internal_keys and filter_name as for
 * lgs_table_get_host.  resident = 0: `file` is borrowed and must stay valid
 * and unchanged in its data blocks until lgs_table_close (a get stages the
 * blocks it reads from it, as lgs_table_get_host does); resident = 1: the
 * whole image is uploaded (16 bytes of slack after it) and `file` may be
 * freed when the call returns.  A table that does not open (short file, bad
 * footer, an index block that does not read) still returns LGS_OK and a
 * handle, with *status = that status; every get on it answers as
 * lgs_table_get_host does for such a table (called 0, that status, verdict
 * LGS_GET_NOTFOUND, all offsets 0).  A filter block that does not read is
 * dropped (table.c:71-72).  The handle belongs to the calling thread's device
 * (lgs_set_device); a later call from a thread set to another device returns
 * LGS_EINVAL.  A handle is read-only once open: any number of threads may
 * call lgs_table_get / lgs_table_get_dev / lgs_table_info on it at once.
 *
 * lgs_table_close frees the resident memory on the stream it was allocated on
 * and waits for that stream alone; no call of this group synchronises the
 * whole device.  No get on the handle may be in flight.  NULL is a no-op.
 *
 * lgs_table_info: any output may be NULL.  *index_bytes / *filter_bytes: the
 * decoded blocks' lengths (0: none); *device_bytes: the memory the handle
 * holds on the device (from its first scan on, the index entry list too).
 *
 * lgs_table_get: lgs_table_get_host's contract, word for word, minus the open
 * arguments.  Between the index seek and the block read it differs inside:
 * the distinct blocks are numbered on the device, by the offset of the index
 * entry a query found rather than by the (offset, size) that entry carries,
 * in file order whatever the order of the queries; two index entries that
 * carry the same handle are read as two blocks, which changes no per-query
 * output.  One read-back of 32 bytes (the number of distinct blocks, the room
 * their contents take, the largest room, an error flag) sizes the block read;
 * a borrowed image's call also fetches the distinct handles to stage their
 * byte ranges.  A Snappy block's room is capped at 2^32 - 16 bytes as well.
 *
 * lgs_table_get_dev: the same with the keys and every per-query result in
 * device memory (d_out_key_off / d_out_val_off: nq + 1 each); *out_needed
 * stays a host word.  Resident tables only: LGS_EINVAL otherwise.  d_keys
 * must be readable 16 bytes past its end.  The work is queued on `stream`,
 * which the call synchronises twice itself, to size the block read and to
 * learn the results' total; the device outputs are complete on `stream` (not
 * necessarily on the host) when it returns.  LGS_ENOSPC as above: d_called
 * and d_status are written, d_out is not.  Scratch comes from the library's
 * stream-ordered pool: per query 68 bytes, per byte of the decoded index block
 * 12, then what the block read and the results take. */
typedef struct lgs_table lgs_table;
int lgs_table_open_host(const uint8_t *file, uint64_t file_len, int paranoid_checks,
                        int internal_keys, const char *filter_name, int resident,
                        lgs_table **table, uint8_t *status);
void lgs_table_close(lgs_table *table);
int lgs_table_info(const lgs_table *table, uint8_t *status, int *resident,
                   uint64_t *index_bytes, uint64_t *filter_bytes, uint64_t *device_bytes);
int lgs_table_get(lgs_table *table, int verify_checksums, const uint8_t *keys,
                  const uint64_t *key_off, const uint32_t *key_len, uint32_t nq,
                  uint8_t *called, uint8_t *status, uint8_t *verdict, uint8_t *out,
                  size_t out_cap, uint64_t *out_key_off, uint64_t *out_val_off,
                  size_t *out_needed);
int lgs_table_get_dev(lgs_table *table, int verify_checksums, const uint8_t *d_keys,
                      const uint64_t *d_key_off, const uint32_t *d_key_len, uint32_t nq,
                      uint8_t *d_called, uint8_t *d_status, uint8_t *d_verdict,
                      uint8_t *d_out, size_t out_cap, uint64_t *d_out_key_off,
                      uint64_t *d_out_val_off, size_t *out_needed, void *stream);

/* ---- forward scans ----
 *
 * The table iterator's forward half: ldb_tableiter_create, then first or
 * seek, then next until invalid.  Blocks in, the entries out flat as (keys,
 * key_off, key_len, vals, val_off, val_len): the layout lgs_block_cut_dev,
 * lgs_block_emit_dev and lgs_table_build_host take, so build(scan(table)) is
 * the table again.
 *
 * A forward scan of one block is ldb_blockiter_first + ldb_blockiter_next
 * until invalid (block.c:247-296, 411-415).  A block under 4 bytes or with a
 * restart count that does not fit is an error iterator (LGS_ST_CORRUPT, no
 * entries); one with 0 restarts is empty (LGS_ST_OK).  Otherwise the walk
 * begins at restart[0], clamped to the restart array's offset, and parses
 * entry after entry up to that offset; it ends LGS_ST_CORRUPT at the first
 * entry that does not decode, whose `shared` exceeds the previous key's
 * length, or (internal_keys) whose key has under 8 bytes, the entries before
 * it delivered.  The restart array plays no other part, and keys are
 * delivered as parsed: their order is not checked.
 *
 * Blocks: d_blocks, d_block_off, d_block_len and the optional d_block_status
 * as for lgs_block_seek_dev; block_bytes: at least the sum of d_block_len
 * (under 3 * 2^31).  d_walk_from / d_emit_from (NULL, or 0xffffffff for a
 * block: not given): the offset in block b where its walk begins instead of
 * restart[0], and the first offset whose entry is delivered -- how a scan
 * follows a seek, which goes on parsing from the restart run it chose.
 *
 * Two device calls, because the host needs the totals between them to size
 * the outputs.  lgs_block_entries_count_dev writes d_entry_first (nblocks + 1:
 * each block's first entry number, the total last), d_status (nblocks) and
 * d_counts[4] = {entries, key bytes, value bytes, longest key}.
 * lgs_block_entries_emit_dev, given n = d_counts[0], rebuilds every key in
 * full and writes d_keys (d_counts[1] + 16 bytes), d_key_off (n + 1), d_key_len
 * (n), d_vals (d_counts[2] + 16), d_val_off (n + 1), d_val_len (n): the 16
 * bytes meet the builder's "readable 16 bytes past the end".  Both take the
 * same lgs_block_entries_scratch(nblocks, block_bytes) bytes of device
 * scratch (12 + 8 bytes per possible entry, a third of block_bytes), left
 * alone between them, and both are asynchronous on `stream`.  nblocks = 0 and
 * blocks without entries are fine.  The work is linear in the block bytes
 * plus the bytes delivered, whatever the blocks hold.
 *
 * lgs_block_entries_host: host arrays in and out (a pooled context, one
 * synchronisation between the two calls, scratch sized by the entries found).
 * entry_first and status are always written, needed[3] = {entries, key bytes,
 * value bytes}; LGS_ENOSPC when entry_cap, key_cap or val_cap is smaller, and
 * then no entry is written. */
size_t lgs_block_entries_scratch(uint32_t nblocks, uint64_t block_bytes);
int lgs_block_entries_count_dev(const uint8_t *d_blocks, const uint64_t *d_block_off,
                                const uint32_t *d_block_len, const uint8_t *d_block_status,
                                uint32_t nblocks, uint64_t block_bytes,
                                const uint32_t *d_walk_from, const uint32_t *d_emit_from,
                                int internal_keys, uint32_t *d_entry_first, uint8_t *d_status,
                                uint64_t *d_counts, void *d_scratch, size_t scratch_bytes,
                                void *stream);
int lgs_block_entries_emit_dev(const uint8_t *d_blocks, const uint64_t *d_block_off,
                               const uint32_t *d_block_len, const uint8_t *d_block_status,
                               uint32_t nblocks, uint64_t block_bytes,
                               const uint32_t *d_walk_from, const uint32_t *d_emit_from,
                               int internal_keys, uint32_t n, uint8_t *d_keys,
                               uint64_t *d_key_off, uint32_t *d_key_len, uint8_t *d_vals,
                               uint64_t *d_val_off, uint32_t *d_val_len, void *d_scratch,
                               size_t scratch_bytes, void *stream);
int lgs_block_entries_host(const uint8_t *blocks, const uint64_t *block_off,
                           const uint32_t *block_len, const uint8_t *block_status,
                           uint32_t nblocks, const uint32_t *walk_from, const uint32_t *emit_from,
                           int internal_keys, uint32_t *entry_first, uint8_t *status,
                           uint8_t *keys, size_t key_cap, uint64_t *key_off, uint32_t *key_len,
                           uint8_t *vals, size_t val_cap, uint64_t *val_off, uint32_t *val_len,
                           uint32_t entry_cap, uint64_t *needed);

/* A forward scan of an opened table: two_level_iterator.c over the block
 * scan, with table.c:229-300 as the block function.  The index block's
 * entries are walked as above; each value goes through ldb_handle_import
 * (LGS_ST_CORRUPT for that block when it is no handle), then the block is read
 * (a failure is that read's status).  A block that yields an error, or ends
 * in one, is skipped and the scan goes on (ldb_twoiter_skip_forward); the
 * scan's final status is the index walk's own when that is not LGS_ST_OK,
 * else the first block status in index order that is not (ldb_twoiter_saverr
 * keeps the first).
 *
 * One call delivers a window of index entries [b0, b0 + max_blocks): b0 =
 * first_block, or with has_start the block ldb_twoiter_seek's index seek
 * names for start[0 .. start_len), where a fresh data iterator then seeks;
 * the window's first block is walked from the restart run that seek chose
 * and delivered from the entry it found (nothing, and the seek's status, when
 * it found none), every later block from its first entry.  Results: the entry
 * arrays above; block_entry_first (max_blocks + 1) and block_status
 * (max_blocks) per block of the window; *blocks_done; *next_block, the
 * first_block of the next call; *at_end; *index_status, the index walk's
 * status, meaningful once *at_end.  needed[4] = {entries, key bytes, value
 * bytes, blocks}: LGS_ENOSPC when a capacity is smaller (no entry is written;
 * enlarge the buffers or shrink the window).  needed[3] is set only for a seek
 * into a damaged index block that finds an entry the walk from restart[0]
 * does not visit: the entries from there to where the two walks meet are one
 * window, whatever max_blocks says.  A table that did not open has no
 * iterator: no blocks, *at_end, *index_status = its status.
 *
 * The first scan of a handle builds its index entry list (positions, decoded
 * handles, the walk's end status) once, under std::call_once, from the
 * handle's pool; lgs_table_info counts it in *device_bytes from then on.  Any
 * number of threads may scan one handle at once.  Read-backs per call: the
 * window's room (a resident image; a borrowed one is planned on the host),
 * then the counts; with has_start the index seek's entry first.  No call
 * synchronises the whole device.
 *
 * lgs_table_scan_dev: every array in device memory, queued on `stream` (which
 * the call synchronises itself for the read-backs) and complete on it when
 * the call returns; key_cap and val_cap include the 16 spare bytes and needed
 * reports them, so the results are lgs_block_cut_dev's input as they stand.
 * start and the scalar results stay host words.  Resident tables only:
 * LGS_EINVAL otherwise. */
int lgs_table_scan(lgs_table *table, int verify_checksums, const uint8_t *start,
                   uint32_t start_len, int has_start, uint32_t first_block, uint32_t max_blocks,
                   uint8_t *keys, size_t key_cap, uint64_t *key_off, uint32_t *key_len,
                   uint8_t *vals, size_t val_cap, uint64_t *val_off, uint32_t *val_len,
                   uint32_t entry_cap, uint32_t *block_entry_first, uint8_t *block_status,
                   uint32_t *blocks_done, uint32_t *next_block, int *at_end,
                   uint8_t *index_status, uint64_t *needed);
int lgs_table_scan_dev(lgs_table *table, int verify_checksums, const uint8_t *start,
                       uint32_t start_len, int has_start, uint32_t first_block,
                       uint32_t max_blocks, uint8_t *d_keys, size_t key_cap, uint64_t *d_key_off,
                       uint32_t *d_key_len, uint8_t *d_vals, size_t val_cap, uint64_t *d_val_off,
                       uint32_t *d_val_len, uint32_t entry_cap, uint32_t *d_block_entry_first,
                       uint8_t *d_block_status, uint32_t *blocks_done, uint32_t *next_block,
                       int *at_end, uint8_t *index_status, uint64_t *needed, void *stream);

/* Merging sorted runs: the forward half of lcdb's merging iterator
 * (src/table/merger.c) and the drop loop of ldb_do_compaction_work
 * (src/db_impl.c:1363-1397), on entries in the layout the scans above deliver
 * and lgs_block_cut_dev takes.  With it scan -> merge -> build stays in device
 * memory.
 *
 * A run is the six arrays of lgs_block_entries_emit_dev / lgs_table_scan_dev
 * plus n: uint64 offsets, uint32 lengths, keys and vals readable 16 bytes past
 * their end.  The lgs_run array itself is host memory; for the _dev calls its
 * pointers are device pointers.  0 <= nruns <= LGS_MERGE_MAX_RUNS (more:
 * LGS_EINVAL), under 2^31 entries in all, per-entry sizes as the builder's.
 *
 * Order: what ldb_mergeiter_first followed by ldb_mergeiter_next until
 * invalid delivers over children positioned on the runs.  The comparator is
 * bytewise (internal_keys = 0, comparator.c:44-88) or the internal-key
 * comparator (internal_keys = 1, dbformat.c:232-285: the user key, all but
 * the last 8 bytes, bytewise; then the trailing fixed64 tag (seq << 8) | type,
 * descending).  ldb_mergeiter_find_smallest (merger.c:107-128) replaces its
 * candidate only on a strict `<`: among equal keys the lowest-numbered run's
 * entry comes first, and within a run the order is the run's own.  Every entry
 * of every run is delivered; equal keys are not collapsed.
 *
 * Preconditions: every run is non-decreasing under the comparator, and with
 * internal_keys every key has at least 8 bytes (the builder's contract; the
 * reference asserts it).  The plan checks both with a compare of each entry
 * and its predecessor: d_counts[5] is the lowest-numbered offending run, or
 * ~0 when there is none.  When it is set the other counts and everything
 * lgs_merge_emit_dev writes are undefined (but inside the buffers the counts
 * size); lgs_merge_host returns LGS_EINVAL and writes nothing.  A tag whose
 * type byte is above 1 is not an error of the call: ldb_put cannot write one,
 * but table files can hold them and lcdb's repairer keeps such tables.
 *
 * Drop rule (drop = 1, internal_keys = 1 only; db_impl.c:1363-1397), walking
 * the merged order.  An entry whose type byte is above 1 fails
 * ldb_pkey_import (dbformat.c:86-107), the other way into "do not hide error
 * keys" (:1363-1367): it is never dropped, and lcdb forgets the current user
 * key, so the entry behind it counts as a first occurrence.  For the others
 * last_seq is LDB_MAX_SEQUENCE (2^56 - 1) at the first entry of a user key
 * and behind an unparsable entry, otherwise the sequence of the entry just
 * before, dropped or not.  An entry is dropped when last_seq <=
 * smallest_snapshot (A), or else when it is a deletion (type 0) with
 * sequence <= smallest_snapshot and drop_deletions is set.  The merge order
 * is the comparator's, by the raw tag, whatever the type byte.
 * drop_deletions stands for
 * ldb_compaction_is_base_level_for_key, which the caller asserts for the
 * whole call: a caller whose answer differs by key gives the levels below
 * the output to lgs_merge_plan_version_dev (below), which answers per key.
 * With drop = 0 nothing is dropped, and smallest_snapshot and
 * drop_deletions are ignored.
 *
 * Two device calls, as lgs_block_cut_dev / _emit_dev, because the host sizes
 * the outputs between them.  lgs_merge_plan_dev orders the entries, applies
 * the rule and writes d_counts[8] = {entries kept, key bytes, value bytes,
 * longest key, entries dropped, first unsorted-or-short-key run or ~0, 0, 0}.
 * lgs_merge_emit_dev, given n_out = d_counts[0], writes d_keys (d_counts[1] +
 * 16 bytes), d_key_off (n_out + 1), d_key_len (n_out), d_vals (d_counts[2] +
 * 16), d_val_off (n_out + 1), d_val_len (n_out) -- lgs_block_cut_dev's input
 * as they stand -- and per kept entry the run and the position in it that it
 * came from, d_src_run and d_src_index (n_out each).  Both take the same runs
 * (the emit copies from the addresses the plan saw) and the same
 * lgs_merge_scratch(n_total, nruns) bytes of device scratch (about 85 bytes
 * per input entry), left alone between them, and both are asynchronous on
 * `stream`.  The work is ceil(log2 nruns) passes of a binary
 * search per entry, then one copy of the kept bytes.
 *
 * lgs_merge_host: host arrays in and out (a pooled context, one
 * synchronisation between plan and emit).  needed[5] = {entries kept, key
 * bytes, value bytes, longest key, entries dropped}; LGS_ENOSPC when
 * entry_cap, key_cap or val_cap is smaller, and then no entry is written.
 * key_off and val_off take entry_cap + 1 values. */
typedef struct lgs_run {
  const uint8_t *keys;
  const uint64_t *key_off;
  const uint32_t *key_len;
  const uint8_t *vals;
  const uint64_t *val_off;
  const uint32_t *val_len;
  uint32_t n;
} lgs_run;
#define LGS_MERGE_MAX_RUNS 64
size_t lgs_merge_scratch(uint32_t n_total, uint32_t nruns);
int lgs_merge_plan_dev(const lgs_run *runs, uint32_t nruns, int internal_keys, int drop,
                       uint64_t smallest_snapshot, int drop_deletions, uint64_t *d_counts,
                       void *d_scratch, size_t scratch_bytes, void *stream);
int lgs_merge_emit_dev(const lgs_run *runs, uint32_t nruns, uint32_t n_out, uint8_t *d_keys,
                       uint64_t *d_key_off, uint32_t *d_key_len, uint8_t *d_vals,
                       uint64_t *d_val_off, uint32_t *d_val_len, uint32_t *d_src_run,
                       uint32_t *d_src_index, void *d_scratch, size_t scratch_bytes,
                       void *stream);
int lgs_merge_host(const lgs_run *runs, uint32_t nruns, int internal_keys, int drop,
                   uint64_t smallest_snapshot, int drop_deletions, uint8_t *keys, size_t key_cap,
                   uint64_t *key_off, uint32_t *key_len, uint8_t *vals, size_t val_cap,
                   uint64_t *val_off, uint32_t *val_len, uint32_t *src_run, uint32_t *src_index,
                   uint32_t entry_cap, uint64_t *needed);

/* The same plan for a compaction inside a version: the two
 * pieces of ldb_do_compaction_work's loop (db_impl.c:1352-1425) that depend on
 * the levels below the output.  Internal keys and the drop rule are implied.
 *
 * levels: a host array of nlevels <= LGS_VERSION_MAX_LEVELS file lists, levels
 * output + 1 (the compaction's level + 2) to 6 in that order; all of it, keys
 * included, is host memory and is copied before the call returns.  Within a
 * level the files are in the level's order: disjoint, `largest` strictly
 * increasing under the internal comparator.  Every key has at least 8 bytes
 * and a level has under 2^31 files (else LGS_EINVAL, as for nlevels above the
 * maximum).  nlevels = 0: no stops, every key at base level, which is
 * lgs_merge_plan_dev(internal_keys = 1, drop = 1, drop_deletions = 1).
 *
 * Base level: where the drop rule above reads drop_deletions, this plan reads
 * ldb_compaction_is_base_level_for_key (version_set.c:2289-2321) of the
 * entry's user key: in every level the first file whose largest user key is
 * >= the key does not exist or has a smallest user key above it.
 *
 * Stops: ldb_compaction_should_stop_before (version_set.c:2324-2351) runs
 * before every entry of the merged order, kept or not, against levels[0] with
 * limit max_grandparent_overlap (file sizes sum to under 2^63: the caller's
 * contract, lcdb's overlapped_bytes is an int64_t).  Files passed by the first
 * key cost nothing.  A stop closes the output file only when one is open, so
 * kept entry k > 0 is a forced file start exactly when a stop lies behind the
 * position of kept entry k - 1 and not behind its own.  d_counts[6] is the
 * number of forced starts; lgs_merge_stops_dev, after the plan and with the
 * same scratch, writes the n_out = d_counts[0] flags (uint32, flag 0 is 0) for
 * lgs_tables_build_forced_dev.  lgs_merge_emit_dev is used as it is, with
 * this plan's scratch.
 *
 * lgs_merge_version_scratch(n_total, nruns, files in all levels, bytes of
 * all their keys) sizes the scratch.  The plan synchronises `stream` before it
 * returns (the levels are uploaded from the caller's memory). */
typedef struct lgs_level_file {
  const uint8_t *smallest;
  uint32_t smallest_len;
  const uint8_t *largest;
  uint32_t largest_len;
  uint64_t file_size;
} lgs_level_file;
typedef struct lgs_level {
  const lgs_level_file *files;
  uint32_t n;
} lgs_level;
#define LGS_VERSION_MAX_LEVELS 5
size_t lgs_merge_version_scratch(uint32_t n_total, uint32_t nruns, uint64_t level_files,
                                 uint64_t level_key_bytes);
int lgs_merge_plan_version_dev(const lgs_run *runs, uint32_t nruns, uint64_t smallest_snapshot,
                               const lgs_level *levels, uint32_t nlevels,
                               uint64_t max_grandparent_overlap, uint64_t *d_counts,
                               void *d_scratch, size_t scratch_bytes, void *stream);
int lgs_merge_stops_dev(uint32_t n_total, uint32_t n_out, uint32_t *d_forced,
                        const void *d_scratch, size_t scratch_bytes, void *stream);

/* Devices and diagnostics. */
/* The drop-in's current footprint: pinned and device bytes held by its
   staging slots, the number of slots created (all devices) and the bytes of
   one slot's arena.  The totals never exceed slots * slot_bytes. */
int lgs_dropin_footprint(size_t *pinned, size_t *device, uint32_t *slots,
                         size_t *slot_bytes);

/* Stop the drop-in's resident service waves (every device), wait until they
   have left, and send drop-in calls through the launch path (one kernel and
   one stream synchronisation per call) until lgs_service_resume().  The
   waves otherwise stay while calls keep coming and leave
   LGS_SERVICE_IDLE_US (default 2 ms) after the last call from any thread;
   an application that synchronises the whole device under sustained
   drop-in traffic (hipDeviceSynchronize, hipFree) brackets that with these
   two calls.  Calls in flight complete (through the launch path if the
   waves left first); results are the same either way. */
int lgs_service_quiesce(void);
int lgs_service_resume(void);

/* Process-wide kernel choices (A/B and tests; the defaults pick by batch):
     "decoder": "auto" | "ring" | "wave"
                "auto": batches of >= 28 672 blocks take the lane-per-block
                route, smaller ones the wave-per-block decoder; "ring" and
                "wave" force one of the two for every batch size.  The
                lane-per-block route is decode_pair_kernel: 64 blocks per
                workgroup, a lane per block in each of two waves, one parsing
                tags and refilling the input rings, one moving bytes and
                flushing (outputs up to 16 MiB a block; larger ones go by
                their size class).
                A batch whose largest output is over the 4 KiB class is first
                split by size class on the device ("split" below), under
                "auto" and "ring" alike; the forced kernel then takes
                the 4 KiB class only, and the 16 KiB class and the outputs
                above it run their own decoders.
     "wide":    "walk"  (decoder of outputs over 16 KiB: the one-tag walk)
     "split":   "1" | "0"  (size-class split of mixed batches, see above)
     "service": "1" | "0"  (the drop-in's resident waves)
     "verify_overlap": "1" | "0"  (table reads: CRC pass beside the decoder)
   Initial values: LGS_DECODE_KERNEL, LGS_NO_SPLIT=1, LGS_DROPIN_SERVICE,
   LGS_VERIFY_OVERLAP=0, read once at load.
   LGS_EINVAL for an unknown name or value.  (The decoders that lost their
   A/B -- "decoder" "quad", "ops", "group" and "chain", "wide" "trips" and
   "group" --
   exist only in the test-only probe library; this library
   rejects them.) */
int lgs_set_option(const char *name, const char *value);

/* HBM yardstick, not part of the codec: copies `bytes` (a multiple of 16)
   from d_src to d_dst (both 16-byte aligned device pointers) with a
   16-bytes-per-lane streaming kernel, asynchronously on `stream`.  bench.py
   times it to report the device's achievable HBM rate beside the 8 TB/s
   spec peak. */
int lgs_hbm_copy_dev(void *d_dst, const void *d_src, size_t bytes, void *stream);

int lgs_device_count(void);
int lgs_set_device(int device);  /* device used by the calling thread */
const char *lgs_last_error(void);
const char *lgs_version(void);

#ifdef __cplusplus
}
#endif

#endif /* LCDB_GPU_SNAPPY_H */
