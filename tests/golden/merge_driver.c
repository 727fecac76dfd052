/*
 * merge_driver.c -- lcdb's own merging iterator and its own compaction
 * (src/table/merger.c, src/db_impl.c, unchanged) as the source of
 * tests/golden/merge.bin.  Compiled by tests/golden/make_merge_golden.py
 * against the reference's headers and oracle/_ref/lcdb/liblcdb_core.a +
 * refsnappy.o; test infrastructure only, never linked into the product.
 *
 * usage: merge_driver build CASE OUT.ldb
 *          (a table by ldb_tablegen_*; the case file of
 *           table_golden_driver.c: block_size, restart_interval, compression,
 *           bits_per_key, internal_keys, n, then per entry key length, key,
 *           value length, value; little-endian u32s)
 *        merge_driver merge INTERNAL OUT T1.ldb [T2.ldb ...]
 *          (ldb_tableiter_create per table, ldb_mergeiter_create over them,
 *           first + next until invalid.  OUT: i32 final status, u32 entries,
 *           then per entry key length, key, value length, value)
 *        merge_driver --time INTERNAL REPS T1.ldb [T2.ldb ...]
 *          (that loop REPS times over; prints the best pass's nanoseconds
 *           per entry)
 *        merge_driver compact DBDIR SCRIPT OUTDIR
 *          (a fresh DB with default options and no compression; the script's
 *           operations; then ldb_test_compact_range at level 0 and at level
 *           1.  Before and after each of the two the live tables are copied
 *           to OUTDIR/stage<k>/ and the "leveldb.sstables" property to
 *           OUTDIR/stage<k>.txt, k = 0, 1, 2.  Script: u32 operations, then
 *           per operation u32 kind: 0 put (key length, key, value length,
 *           value), 1 delete (key length, key), 2 ldb_test_compact_memtable,
 *           3 ldb_snapshot, never released)
 *        merge_driver repair DBDIR SCRIPT OUTDIR
 *          (DBDIR holds nothing but table files <number>.ldb written by the
 *           `build` mode: ldb_repair puts them at level 0 and sets the last
 *           sequence to the largest parsable one in them; then `compact` as
 *           it stands: the open, the script, the two steps and the stage
 *           dumps.  tests/golden/make_merge_sweep_golden.py)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "db_impl.h"
#include "dbformat.h"
#include "table/iterator.h"
#include "table/merger.h"
#include "table/table.h"
#include "table/table_builder.h"
#include "util/bloom.h"
#include "util/comparator.h"
#include "util/env.h"
#include "util/options.h"
#include "util/slice.h"
#include "util/status.h"

#define MAX_TABLES 64

static unsigned long
rd32(FILE *f) {
  unsigned char b[4];

  if (fread(b, 1, 4, f) != 4) {
    fprintf(stderr, "short input file\n");
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

static unsigned char *
rdblob(FILE *f, unsigned long *n) {
  unsigned char *p;

  *n = rd32(f);
  p = malloc(*n + 1);

  if (*n && fread(p, 1, *n, f) != *n) {
    fprintf(stderr, "short input file\n");
    exit(2);
  }

  return p;
}

static int
do_build(const char *case_path, const char *out_path) {
  ldb_comparator_t icmp;
  ldb_bloom_t user_bloom, ifp;
  ldb_dbopt_t options;
  ldb_tablegen_t *tb;
  ldb_wfile_t *file;
  unsigned long bits, internal, n, i;
  FILE *f;
  int rc;

  if ((f = fopen(case_path, "rb")) == NULL)
    return 2;

  options = *ldb_dbopt_default;
  options.block_size = rd32(f);
  options.block_restart_interval = (int)rd32(f);
  options.compression = rd32(f) ? LDB_SNAPPY_COMPRESSION : LDB_NO_COMPRESSION;
  bits = rd32(f);
  internal = rd32(f);
  n = rd32(f);

  options.comparator = ldb_bytewise_comparator;
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

  rc = ldb_truncfile_create(out_path, &file);
  if (rc != LDB_OK) {
    fprintf(stderr, "%s: %s\n", out_path, ldb_strerror(rc));
    return 1;
  }

  tb = ldb_tablegen_create(&options, file);

  for (i = 0; i < n; i++) {
    unsigned long kn, vn;
    unsigned char *kp = rdblob(f, &kn);
    unsigned char *vp = rdblob(f, &vn);
    ldb_slice_t key = ldb_slice(kp, kn);
    ldb_slice_t val = ldb_slice(vp, vn);

    ldb_tablegen_add(tb, &key, &val);

    free(kp);
    free(vp);
  }

  rc = ldb_tablegen_finish(tb);
  if (rc == LDB_OK)
    rc = ldb_wfile_close(file);

  ldb_tablegen_destroy(tb);
  ldb_wfile_destroy(file);
  fclose(f);

  return rc == LDB_OK ? 0 : 1;
}

/* One pass of the merging loop; out == NULL: count only. */
static unsigned long
run_merge(const ldb_comparator_t *cmp,
          ldb_table_t **tables,
          int n,
          const ldb_readopt_t *ropt,
          FILE *out,
          unsigned long *sink) {
  ldb_iter_t *children[MAX_TABLES];
  ldb_iter_t *it;
  unsigned long count = 0;
  int i;

  for (i = 0; i < n; i++)
    children[i] = ldb_tableiter_create(tables[i], ropt);

  it = ldb_mergeiter_create(cmp, children, n);

  if (out != NULL) {
    wr32(out, 0);
    wr32(out, 0);
  }

  for (ldb_iter_first(it); ldb_iter_valid(it); ldb_iter_next(it)) {
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
      *sink += k.size + v.size + (v.size ? ((unsigned char *)v.data)[v.size - 1] : 0);
    }

    count++;
  }

  if (out != NULL) {
    long end = ftell(out);

    fseek(out, 0, SEEK_SET);
    wr32(out, (unsigned long)ldb_iter_status(it));
    wr32(out, count);
    fseek(out, end, SEEK_SET);
  }

  ldb_iter_destroy(it);

  return count;
}

static int
do_merge(int timing, int internal, const char *arg, int n, char **paths) {
  ldb_comparator_t icmp;
  ldb_dbopt_t options;
  ldb_readopt_t ropt;
  ldb_rfile_t *files[MAX_TABLES];
  ldb_table_t *tables[MAX_TABLES];
  unsigned long sink = 0, count = 0;
  int i, rc;

  if (n > MAX_TABLES)
    return 2;

  options = *ldb_dbopt_default;
  options.block_cache = NULL;
  options.comparator = ldb_bytewise_comparator;
  options.filter_policy = NULL;

  if (internal) {
    ldb_ikc_init(&icmp, ldb_bytewise_comparator);
    options.comparator = &icmp;
  }

  ropt = *ldb_readopt_default;
  ropt.verify_checksums = 1;

  for (i = 0; i < n; i++) {
    uint64_t size;

    rc = ldb_file_size(paths[i], &size);
    if (rc == LDB_OK)
      rc = ldb_randfile_create(paths[i], &files[i], 0);
    if (rc == LDB_OK)
      rc = ldb_table_open(&options, files[i], size, &tables[i]);
    if (rc != LDB_OK) {
      fprintf(stderr, "%s: %s\n", paths[i], ldb_strerror(rc));
      return 1;
    }
  }

  if (timing) {
    unsigned long reps = strtoul(arg, NULL, 10), r;
    double best = 0.0;

    for (r = 0; r < reps; r++) {
      struct timespec t0, t1;
      double ns;

      clock_gettime(CLOCK_MONOTONIC, &t0);
      count = run_merge(options.comparator, tables, n, &ropt, NULL, &sink);
      clock_gettime(CLOCK_MONOTONIC, &t1);

      ns = (t1.tv_sec - t0.tv_sec) * 1e9 + (t1.tv_nsec - t0.tv_nsec);
      if (r == 0 || ns < best)
        best = ns;
    }

    printf("tables=%d entries=%lu reps=%lu sink=%lu ns_per_entry=%.1f ns_per_merge=%.0f\n",
           n, count, reps, sink, count ? best / count : 0.0, best);
  } else {
    FILE *out = fopen(arg, "wb");

    if (out == NULL)
      return 2;

    count = run_merge(options.comparator, tables, n, &ropt, out, &sink);
    fclose(out);

    printf("tables=%d entries=%lu\n", n, count);
  }

  for (i = 0; i < n; i++) {
    ldb_table_destroy(tables[i]);
    ldb_rfile_destroy(files[i]);
  }

  return 0;
}

static void
dump_stage(ldb_t *db, const char *dbdir, const char *outdir, int stage) {
  char cmd[4096];
  char path[2048];
  char *text = NULL;
  int level;
  FILE *f;

  /* A compaction that keeps nothing leaves no table file behind. */
  sprintf(cmd,
          "mkdir -p '%s/stage%d' && for f in '%s'/*.ldb; do "
          "[ -e \"$f\" ] || continue; cp \"$f\" '%s/stage%d/' || exit 1; done",
          outdir, stage, dbdir, outdir, stage);

  if (system(cmd) != 0) {
    fprintf(stderr, "copy failed: %s\n", cmd);
    exit(1);
  }

  sprintf(path, "%s/stage%d.txt", outdir, stage);

  if (!ldb_property(db, "leveldb.sstables", &text) || (f = fopen(path, "wb")) == NULL) {
    fprintf(stderr, "no sstables property\n");
    exit(1);
  }

  fputs(text, f);
  ldb_free(text);

  for (level = 0; level < 4; level++) {
    char name[64];

    sprintf(name, "leveldb.num-files-at-level%d", level);

    if (!ldb_property(db, name, &text)) {
      fprintf(stderr, "no %s property\n", name);
      exit(1);
    }

    fprintf(f, "files-at-level %d %s\n", level, text);
    ldb_free(text);
  }

  fclose(f);
}

static int
do_compact(int repair, const char *dbdir, const char *script, const char *outdir) {
  ldb_dbopt_t options;
  unsigned long nops, i;
  ldb_t *db;
  FILE *f;
  int rc;

  if ((f = fopen(script, "rb")) == NULL)
    return 2;

  options = *ldb_dbopt_default;
  options.create_if_missing = 1;
  options.compression = LDB_NO_COMPRESSION;

  if (repair) {
    rc = ldb_repair(dbdir, &options);
    if (rc != LDB_OK) {
      fprintf(stderr, "repair of %s: %s\n", dbdir, ldb_strerror(rc));
      return 1;
    }
  }

  rc = ldb_open(dbdir, &options, &db);
  if (rc != LDB_OK) {
    fprintf(stderr, "%s: %s\n", dbdir, ldb_strerror(rc));
    return 1;
  }

  nops = rd32(f);

  for (i = 0; i < nops && rc == LDB_OK; i++) {
    unsigned long kind = rd32(f);

    if (kind == 0 || kind == 1) {
      unsigned long kn, vn = 0;
      unsigned char *kp = rdblob(f, &kn);
      unsigned char *vp = kind == 0 ? rdblob(f, &vn) : NULL;
      ldb_slice_t key = ldb_slice(kp, kn);
      ldb_slice_t val = ldb_slice(vp, vn);

      if (kind == 0)
        rc = ldb_put(db, &key, &val, ldb_writeopt_default);
      else
        rc = ldb_del(db, &key, ldb_writeopt_default);

      free(kp);
      free(vp);
    } else if (kind == 2) {
      rc = ldb_test_compact_memtable(db);
    } else if (kind == 3) {
      (void)ldb_snapshot(db);
    } else {
      return 2;
    }
  }

  fclose(f);

  if (rc != LDB_OK) {
    fprintf(stderr, "operation %lu: %s\n", i, ldb_strerror(rc));
    return 1;
  }

  dump_stage(db, dbdir, outdir, 0);
  ldb_test_compact_range(db, 0, NULL, NULL);
  dump_stage(db, dbdir, outdir, 1);
  ldb_test_compact_range(db, 1, NULL, NULL);
  dump_stage(db, dbdir, outdir, 2);

  /* The snapshots are still held: the process ends without ldb_close. */
  return 0;
}

int
main(int argc, char **argv) {
  if (argc == 4 && strcmp(argv[1], "build") == 0)
    return do_build(argv[2], argv[3]);

  if (argc >= 4 && strcmp(argv[1], "merge") == 0)
    return do_merge(0, atoi(argv[2]), argv[3], argc - 4, argv + 4);

  if (argc >= 4 && strcmp(argv[1], "--time") == 0)
    return do_merge(1, atoi(argv[2]), argv[3], argc - 4, argv + 4);

  if (argc == 5 && strcmp(argv[1], "compact") == 0)
    return do_compact(0, argv[2], argv[3], argv[4]);

  if (argc == 5 && strcmp(argv[1], "repair") == 0)
    return do_compact(1, argv[2], argv[3], argv[4]);

  fprintf(stderr, "usage: %s build | merge | --time | compact | repair ... (see the source)\n", argv[0]);

  return 2;
}
