/*
 * table_scan_driver.c -- forward scans of one SSTable by lcdb's own table
 * iterator (src/table/table.c, two_level_iterator.c, block.c, unchanged):
 * ldb_table_open, then per run a fresh ldb_tableiter_create, first or seek,
 * and next until invalid.  Compiled by tests/golden/make_scan_golden.py
 * against the reference's headers and oracle/_ref/lcdb/liblcdb_core.a +
 * refsnappy.o; test infrastructure only, never linked into the product.
 *
 * Case file (little-endian u32s): internal_keys, bits_per_key,
 * paranoid_checks, verify_checksums, n; then per seek: key length, key.
 * internal_keys = 1: the table uses the DB's comparator and filter policy
 * (dbformat.c:206-345), as db_impl.c:455-460 sets them up.
 *
 * Output: i32 rc of ldb_table_open; if it is LDB_OK, n + 1 runs (the full
 * scan, then one per seek): i32 final ldb_iter_status, u32 entries, then per
 * entry u32 key length, key, u32 value length, value.
 *
 * usage: table_scan_driver TABLE.ldb CASE OUT
 *        table_scan_driver --time TABLE.ldb REPS
 *          (the full scan REPS times over with the bytewise comparator and
 *           checksums verified; prints the best pass's nanoseconds per entry)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "dbformat.h"
#include "table/iterator.h"
#include "table/table.h"
#include "util/bloom.h"
#include "util/comparator.h"
#include "util/env.h"
#include "util/options.h"
#include "util/slice.h"
#include "util/status.h"

static unsigned long
rd32(FILE *f) {
  unsigned char b[4];

  if (fread(b, 1, 4, f) != 4) {
    fprintf(stderr, "short case file\n");
    exit(2);
  }

  return b[0] | ((unsigned long)b[1] << 8) | ((unsigned long)b[2] << 16) |
         ((unsigned long)b[3] << 24);
}

static void
wr32(FILE *f, unsigned long v) {
  unsigned char b[4];

  b[0] = v & 255;
  b[1] = (v >> 8) & 255;
  b[2] = (v >> 16) & 255;
  b[3] = (v >> 24) & 255;

  fwrite(b, 1, 4, f);
}

/* One run; out == NULL: count only.  Returns the entries seen. */
static unsigned long
run_scan(const ldb_table_t *table,
         const ldb_readopt_t *ropt,
         const ldb_slice_t *start,
         FILE *out,
         unsigned long *sink) {
  ldb_iter_t *it = ldb_tableiter_create(table, ropt);
  unsigned long count = 0;
  long head = 0;

  if (out != NULL) {
    head = ftell(out);
    wr32(out, 0);
    wr32(out, 0);
  }

  if (start != NULL)
    ldb_iter_seek(it, start);
  else
    ldb_iter_first(it);

  while (ldb_iter_valid(it)) {
    ldb_slice_t k = ldb_iter_key(it);
    ldb_slice_t v = ldb_iter_value(it);

    if (out != NULL) {
      wr32(out, (unsigned long)k.size);
      if (k.size)
        fwrite(k.data, 1, k.size, out);
      wr32(out, (unsigned long)v.size);
      if (v.size)
        fwrite(v.data, 1, v.size, out);
    } else {
      *sink += k.size + v.size + (v.size ? v.data[v.size - 1] : 0);
    }

    count++;
    ldb_iter_next(it);
  }

  if (out != NULL) {
    long end = ftell(out);

    fseek(out, head, SEEK_SET);
    wr32(out, (unsigned long)ldb_iter_status(it));
    wr32(out, count);
    fseek(out, end, SEEK_SET);
  }

  ldb_iter_destroy(it);

  return count;
}

int
main(int argc, char **argv) {
  ldb_comparator_t icmp;
  ldb_bloom_t user_bloom, ifp;
  ldb_dbopt_t options;
  ldb_readopt_t ropt;
  ldb_rfile_t *file;
  ldb_table_t *table;
  unsigned long internal = 0, bits = 0, n = 0, i, reps = 0;
  unsigned char **keys = NULL;
  size_t *lens = NULL;
  uint64_t size;
  int timing, rc;
  FILE *f, *out = NULL;

  timing = argc == 4 && strcmp(argv[1], "--time") == 0;

  if (!timing && argc != 4) {
    fprintf(stderr, "usage: %s TABLE.ldb CASE OUT | --time TABLE.ldb REPS\n", argv[0]);
    return 2;
  }

  options = *ldb_dbopt_default;
  options.block_cache = NULL;
  options.comparator = ldb_bytewise_comparator;
  options.filter_policy = NULL;

  ropt = *ldb_readopt_default;
  ropt.verify_checksums = 1;

  if (timing) {
    argv++;
    reps = strtoul(argv[2], NULL, 10);
  } else {
    if ((f = fopen(argv[2], "rb")) == NULL) {
      fprintf(stderr, "%s: cannot open\n", argv[2]);
      return 2;
    }

    internal = rd32(f);
    bits = rd32(f);
    options.paranoid_checks = (int)rd32(f);
    ropt.verify_checksums = (int)rd32(f);

    if (internal) {
      ldb_ikc_init(&icmp, ldb_bytewise_comparator);
      options.comparator = &icmp;
    }

    if (bits > 0) {
      ldb_bloom_init(&user_bloom, (int)bits);
      options.filter_policy = &user_bloom;
      if (internal) {
        ldb_ifp_init(&ifp, &user_bloom);
        options.filter_policy = &ifp;
      }
    }

    n = rd32(f);
    keys = malloc((n + 1) * sizeof(*keys));
    lens = malloc((n + 1) * sizeof(*lens));

    for (i = 0; i < n; i++) {
      lens[i] = rd32(f);
      keys[i] = malloc(lens[i] + 1);
      if (lens[i] && fread(keys[i], 1, lens[i], f) != lens[i])
        return 2;
    }

    fclose(f);
  }

  rc = ldb_file_size(argv[1], &size);
  if (rc == LDB_OK)
    rc = ldb_randfile_create(argv[1], &file, 0);
  if (rc != LDB_OK) {
    fprintf(stderr, "%s: %s\n", argv[1], ldb_strerror(rc));
    return 1;
  }

  rc = ldb_table_open(&options, file, size, &table);

  if (timing) {
    double best = 0.0;
    unsigned long r, count = 0, sink = 0;

    if (rc != LDB_OK) {
      fprintf(stderr, "open: %s\n", ldb_strerror(rc));
      return 1;
    }

    for (r = 0; r < reps; r++) {
      struct timespec t0, t1;
      double ns;

      clock_gettime(CLOCK_MONOTONIC, &t0);
      count = run_scan(table, &ropt, NULL, NULL, &sink);
      clock_gettime(CLOCK_MONOTONIC, &t1);

      ns = (t1.tv_sec - t0.tv_sec) * 1e9 + (t1.tv_nsec - t0.tv_nsec);
      if (r == 0 || ns < best)
        best = ns;
    }

    printf("entries=%lu reps=%lu sink=%lu ns_per_entry=%.1f ns_per_scan=%.0f\n", count,
           reps, sink, count ? best / count : 0.0, best);

    ldb_table_destroy(table);
    ldb_rfile_destroy(file);
    return 0;
  }

  if ((out = fopen(argv[3], "wb")) == NULL)
    return 2;

  wr32(out, (unsigned long)rc);

  if (rc == LDB_OK) {
    unsigned long sink = 0;

    run_scan(table, &ropt, NULL, out, &sink);

    for (i = 0; i < n; i++) {
      ldb_slice_t k = ldb_slice(keys[i], lens[i]);

      run_scan(table, &ropt, &k, out, &sink);
    }

    ldb_table_destroy(table);
  }

  ldb_rfile_destroy(file);
  fclose(out);

  printf("open=%d runs=%lu\n", rc, n + 1);

  return 0;
}
