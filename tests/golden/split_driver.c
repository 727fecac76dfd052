/*
 * split_driver.c -- lcdb's own table builder cut into compaction's output
 * files, and one real lcdb compaction with several output files, as the
 * source of tests/golden/compact_split.bin.  Compiled by
 * tests/golden/make_split_golden.py against the reference's headers and
 * oracle/_ref/lcdb/liblcdb_core.a + refsnappy.o; test infrastructure only,
 * never linked into the product.
 *
 * usage: split_driver split CASE OUTDIR
 *          (ldb_tablegen_* driven as ldb_do_compaction_work drives it for
 *           every kept entry: open an output table if none is open, add the
 *           entry, close the table once ldb_tablegen_size has reached
 *           max_output_file_size.  The DB clips max_file_size to 1 MiB and
 *           more, so smaller sizes are reachable only here.  CASE: u32
 *           block_size, restart_interval, compression, bits_per_key,
 *           internal_keys, max_output_file_size low and high word, n, then
 *           per entry key length, key, value length, value; little-endian.
 *           Writes OUTDIR/<file index, 6 digits>.ldb and OUTDIR/split.txt,
 *           one line "index entries bytes" per file)
 *        split_driver compact DBDIR SCRIPT OUTDIR
 *          (a fresh DB with max_file_size = 1 MiB and no compression; the
 *           script's operations; then ldb_test_compact_range at level 0.
 *           Before and after it the live tables are copied to
 *           OUTDIR/stage<k>/ and the "leveldb.sstables" property to
 *           OUTDIR/stage<k>.txt, k = 0, 1.  Script: u32 operations, then per
 *           operation u32 kind: 0 put (key length, key, value length, value),
 *           1 delete (key length, key), 2 ldb_test_compact_memtable,
 *           4 close and reopen the DB: recovery writes the log's entries as a
 *           level-0 table whatever the levels below hold)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "db_impl.h"
#include "dbformat.h"
#include "table/table_builder.h"
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
    fprintf(stderr, "short input file\n");
    exit(2);
  }

  return b[0] | ((unsigned long)b[1] << 8) | ((unsigned long)b[2] << 16) |
         ((unsigned long)b[3] << 24);
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
do_split(const char *case_path, const char *outdir) {
  ldb_comparator_t icmp;
  ldb_bloom_t user_bloom, ifp;
  ldb_dbopt_t options;
  ldb_tablegen_t *tb = NULL;
  ldb_wfile_t *file = NULL;
  unsigned long bits, internal, n, i, lo, hi, files = 0;
  uint64_t max_size;
  char path[2048];
  FILE *f, *list;
  int rc = LDB_OK;

  if ((f = fopen(case_path, "rb")) == NULL)
    return 2;

  options = *ldb_dbopt_default;
  options.block_size = rd32(f);
  options.block_restart_interval = (int)rd32(f);
  options.compression = rd32(f) ? LDB_SNAPPY_COMPRESSION : LDB_NO_COMPRESSION;
  bits = rd32(f);
  internal = rd32(f);
  lo = rd32(f);
  hi = rd32(f);
  n = rd32(f);
  max_size = ((uint64_t)hi << 32) | lo;

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

  sprintf(path, "%s/split.txt", outdir);
  if ((list = fopen(path, "wb")) == NULL)
    return 2;

  for (i = 0; i < n && rc == LDB_OK; i++) {
    unsigned long kn, vn;
    unsigned char *kp = rdblob(f, &kn);
    unsigned char *vp = rdblob(f, &vn);
    ldb_slice_t key = ldb_slice(kp, kn);
    ldb_slice_t val = ldb_slice(vp, vn);

    if (tb == NULL) {
      sprintf(path, "%s/%06lu.ldb", outdir, files);
      rc = ldb_truncfile_create(path, &file);
      if (rc != LDB_OK)
        break;
      tb = ldb_tablegen_create(&options, file);
    }

    ldb_tablegen_add(tb, &key, &val);

    free(kp);
    free(vp);

    if (ldb_tablegen_size(tb) >= max_size || i + 1 == n) {
      rc = ldb_tablegen_finish(tb);
      if (rc == LDB_OK)
        rc = ldb_wfile_close(file);

      fprintf(list, "%lu %lu %lu\n", files, (unsigned long)ldb_tablegen_entries(tb),
              (unsigned long)ldb_tablegen_size(tb));

      ldb_tablegen_destroy(tb);
      ldb_wfile_destroy(file);
      tb = NULL;
      files++;
    }
  }

  fclose(list);
  fclose(f);

  if (rc != LDB_OK)
    fprintf(stderr, "%s: %s\n", outdir, ldb_strerror(rc));

  return rc == LDB_OK ? 0 : 1;
}

static void
dump_stage(ldb_t *db, const char *dbdir, const char *outdir, int stage) {
  char cmd[4096];
  char path[2048];
  char *text = NULL;
  FILE *f;

  sprintf(cmd, "mkdir -p '%s/stage%d' && cp '%s'/*.ldb '%s/stage%d/'", outdir, stage, dbdir,
          outdir, stage);

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
  fclose(f);
}

static int
do_compact(const char *dbdir, const char *script, const char *outdir) {
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
  options.max_file_size = 1 << 20;

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
    } else if (kind == 4) {
      ldb_close(db);
      rc = ldb_open(dbdir, &options, &db);
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
  ldb_close(db);

  return 0;
}

int
main(int argc, char **argv) {
  if (argc == 4 && strcmp(argv[1], "split") == 0)
    return do_split(argv[2], argv[3]);

  if (argc == 5 && strcmp(argv[1], "compact") == 0)
    return do_compact(argv[2], argv[3], argv[4]);

  fprintf(stderr, "usage: %s split CASE OUTDIR | compact DBDIR SCRIPT OUTDIR\n", argv[0]);

  return 2;
}
