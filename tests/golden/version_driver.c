/*
 * version_driver.c -- lcdb's compaction loop inside a version: the source of
 * tests/golden/compact_version.bin.  Compiled by
 * tests/golden/make_version_golden.py against the reference's headers and
 * oracle/_ref/lcdb/liblcdb_core.a + refsnappy.o; test infrastructure only,
 * never linked into the product.
 *
 * usage: version_driver loop CASE OUTDIR
 *          (the body of ldb_do_compaction_work's loop, db_impl.c:1352-1425,
 *           over an already merged entry list, around lcdb's own
 *           ldb_compaction_should_stop_before,
 *           ldb_compaction_is_base_level_for_key, ldb_pkey_import and
 *           ldb_tablegen_*.  The compaction, its input version and the
 *           version set are assembled by hand: a compaction at level 0 whose
 *           version holds the case's file lists in levels 2 to 6, all of
 *           level 2 as its grandparents.  max_grandparent_overlap_bytes is
 *           10 * options.max_file_size (version_set.c:57), and the DB clips
 *           that option to 1 MiB and more, so smaller limits are reachable
 *           only here.  CASE, little-endian: u32 block_size,
 *           restart_interval, compression, bits_per_key; u64
 *           max_output_file_size, options.max_file_size, smallest_snapshot;
 *           u32 levels, per level u32 files, per file smallest key, largest
 *           key (u32 length, bytes) and u64 file_size; u32 entries, per
 *           entry key and value.  Writes OUTDIR/<file index, 6 digits>.ldb,
 *           OUTDIR/loop.txt, one line "index entries bytes" per file, and
 *           OUTDIR/flags.txt, one line "stop drop" per entry: what
 *           should_stop_before returned and whether the entry was dropped)
 *        version_driver compact DBDIR SCRIPT OUTDIR
 *          (split_driver's compact mode: a fresh DB with max_file_size =
 *           1 MiB and no compression, the script's operations, then
 *           ldb_test_compact_range at level 0; the live tables and the
 *           "leveldb.sstables" property before and after it go to
 *           OUTDIR/stage<k>/ and OUTDIR/stage<k>.txt.  Script: u32
 *           operations, per operation u32 kind: 0 put (key, value), 1 delete
 *           (key), 2 ldb_test_compact_memtable)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "db_impl.h"
#include "dbformat.h"
#include "table/table_builder.h"
#include "util/bloom.h"
#include "util/buffer.h"
#include "util/comparator.h"
#include "util/env.h"
#include "util/options.h"
#include "util/slice.h"
#include "util/status.h"
#include "util/vector.h"
#include "version_edit.h"
#include "version_set.h"

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

static uint64_t
rd64(FILE *f) {
  uint64_t lo = rd32(f);
  uint64_t hi = rd32(f);

  return lo | (hi << 32);
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

typedef struct output_s {
  ldb_tablegen_t *tb;
  ldb_wfile_t *file;
  unsigned long files;
  FILE *list;
  const char *outdir;
} output_t;

static int
output_finish(output_t *o) {
  int rc = ldb_tablegen_finish(o->tb);

  if (rc == LDB_OK)
    rc = ldb_wfile_close(o->file);

  fprintf(o->list, "%lu %lu %lu\n", o->files,
          (unsigned long)ldb_tablegen_entries(o->tb),
          (unsigned long)ldb_tablegen_size(o->tb));

  ldb_tablegen_destroy(o->tb);
  ldb_wfile_destroy(o->file);

  o->tb = NULL;
  o->files++;

  return rc;
}

static int
do_loop(const char *case_path, const char *outdir) {
  ldb_bloom_t user_bloom, ifp;
  ldb_dbopt_t options;
  ldb_versions_t vset;
  ldb_version_t *ver;
  ldb_compaction_t *c;
  ldb_buffer_t user_key;
  uint64_t smallest_snapshot, last_seq = LDB_MAX_SEQUENCE;
  unsigned long bits, levels, n, i, v;
  int has_user_key = 0;
  char path[2048];
  output_t out;
  FILE *f, *flags;
  int rc = LDB_OK;

  if ((f = fopen(case_path, "rb")) == NULL)
    return 2;

  options = *ldb_dbopt_default;
  options.block_size = rd32(f);
  options.block_restart_interval = (int)rd32(f);
  options.compression = rd32(f) ? LDB_SNAPPY_COMPRESSION : LDB_NO_COMPRESSION;
  bits = rd32(f);

  memset(&vset, 0, sizeof(vset));
  ldb_ikc_init(&vset.icmp, ldb_bytewise_comparator);
  vset.options = &options;
  options.comparator = &vset.icmp;

  if (bits > 0) {
    ldb_bloom_init(&user_bloom, (int)bits);
    ldb_ifp_init(&ifp, &user_bloom);
    options.filter_policy = &ifp;
  }

  ver = ldb_version_create(&vset);
  c = ldb_compaction_create(&options, 0);
  c->input_version = ver;
  c->max_output_file_size = rd64(f);
  options.max_file_size = (size_t)rd64(f);
  smallest_snapshot = rd64(f);

  levels = rd32(f);

  if (levels > LDB_NUM_LEVELS - 2)
    return 2;

  for (v = 0; v < levels; v++) {
    unsigned long files = rd32(f);

    for (i = 0; i < files; i++) {
      ldb_filemeta_t *meta = ldb_filemeta_create();
      unsigned long sn, ln;
      unsigned char *sp = rdblob(f, &sn);
      unsigned char *lp = rdblob(f, &ln);

      ldb_buffer_set(&meta->smallest, sp, sn);
      ldb_buffer_set(&meta->largest, lp, ln);

      meta->number = 1000 * (v + 2) + i;
      meta->file_size = rd64(f);
      meta->refs = 1;

      ldb_vector_push(&ver->files[v + 2], meta);

      if (v == 0)
        ldb_vector_push(&c->grandparents, meta);

      free(sp);
      free(lp);
    }
  }

  sprintf(path, "%s/loop.txt", outdir);
  out.list = fopen(path, "wb");
  sprintf(path, "%s/flags.txt", outdir);
  flags = fopen(path, "wb");

  if (out.list == NULL || flags == NULL)
    return 2;

  out.tb = NULL;
  out.file = NULL;
  out.files = 0;
  out.outdir = outdir;

  ldb_buffer_init(&user_key);

  n = rd32(f);

  for (i = 0; i < n && rc == LDB_OK; i++) {
    unsigned long kn, vn;
    unsigned char *kp = rdblob(f, &kn);
    unsigned char *vp = rdblob(f, &vn);
    ldb_slice_t key = ldb_slice(kp, kn);
    ldb_slice_t val = ldb_slice(vp, vn);
    ldb_pkey_t ikey;
    int stop, drop = 0;

    /* db_impl.c:1354-1360: the stop is asked first and always. */
    stop = ldb_compaction_should_stop_before(c, &key);

    if (stop && out.tb != NULL)
      rc = output_finish(&out);

    /* :1363-1397 */
    if (!ldb_pkey_import(&ikey, &key)) {
      ldb_buffer_reset(&user_key);
      has_user_key = 0;
      last_seq = LDB_MAX_SEQUENCE;
    } else {
      ldb_slice_t cur = ldb_slice(user_key.data, user_key.size);

      if (!has_user_key ||
          ldb_compare(ldb_bytewise_comparator, &ikey.user_key, &cur) != 0) {
        ldb_buffer_set(&user_key, ikey.user_key.data, ikey.user_key.size);
        has_user_key = 1;
        last_seq = LDB_MAX_SEQUENCE;
      }

      if (last_seq <= smallest_snapshot)
        drop = 1;
      else if (ikey.type == LDB_TYPE_DELETION &&
               ikey.sequence <= smallest_snapshot &&
               ldb_compaction_is_base_level_for_key(c, &ikey.user_key))
        drop = 1;

      last_seq = ikey.sequence;
    }

    fprintf(flags, "%d %d\n", stop, drop);

    /* :1399-1425 */
    if (!drop && rc == LDB_OK) {
      if (out.tb == NULL) {
        sprintf(path, "%s/%06lu.ldb", outdir, out.files);
        rc = ldb_truncfile_create(path, &out.file);

        if (rc != LDB_OK)
          break;

        out.tb = ldb_tablegen_create(&options, out.file);
      }

      ldb_tablegen_add(out.tb, &key, &val);

      if (ldb_tablegen_size(out.tb) >= c->max_output_file_size)
        rc = output_finish(&out);
    }

    free(kp);
    free(vp);
  }

  /* :1433-1434 */
  if (rc == LDB_OK && out.tb != NULL)
    rc = output_finish(&out);

  fclose(out.list);
  fclose(flags);
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
  if (argc == 4 && strcmp(argv[1], "loop") == 0)
    return do_loop(argv[2], argv[3]);

  if (argc == 5 && strcmp(argv[1], "compact") == 0)
    return do_compact(argv[2], argv[3], argv[4]);

  fprintf(stderr, "usage: %s loop CASE OUTDIR | compact DBDIR SCRIPT OUTDIR\n", argv[0]);

  return 2;
}
