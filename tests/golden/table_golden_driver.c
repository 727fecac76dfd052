/*
 * table_golden_driver.c -- writes one SSTable with lcdb's own table builder
 * (src/table/table_builder.c, unchanged) from the entries of a case file.
 * Compiled by tests/golden/make_table_golden.py against the reference's
 * headers and oracle/_ref/lcdb/liblcdb_core.a + refsnappy.o; test
 * infrastructure only, never linked into the product.
 *
 * Case file (little-endian u32s): block_size, restart_interval,
 * compression, bits_per_key, internal_keys, n; then per entry: key length,
 * key, value length, value.  internal_keys = 1: the keys are internal keys
 * and the table uses the DB's comparator and filter policy
 * (dbformat.c:206-345), as db_impl.c:455-460 sets them up.
 *
 * usage: table_golden_driver CASE OUT.ldb
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    fprintf(stderr, "short case file\n");
    exit(2);
  }

  return b[0] | ((unsigned long)b[1] << 8) | ((unsigned long)b[2] << 16) |
         ((unsigned long)b[3] << 24);
}

int
main(int argc, char **argv) {
  ldb_comparator_t icmp;
  ldb_bloom_t user_bloom, ifp;
  ldb_dbopt_t options;
  ldb_tablegen_t *tb;
  ldb_wfile_t *file;
  unsigned long bits, internal, n, i;
  FILE *f;
  int rc;

  if (argc != 3 || (f = fopen(argv[1], "rb")) == NULL) {
    fprintf(stderr, "usage: %s CASE OUT.ldb\n", argv[0]);
    return 2;
  }

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

  rc = ldb_truncfile_create(argv[2], &file);
  if (rc != LDB_OK) {
    fprintf(stderr, "%s: %s\n", argv[2], ldb_strerror(rc));
    return 1;
  }

  tb = ldb_tablegen_create(&options, file);

  for (i = 0; i < n; i++) {
    unsigned long kn = rd32(f), vn;
    unsigned char *kp = malloc(kn + 1), *vp;
    ldb_slice_t key, val;

    if (kn && fread(kp, 1, kn, f) != kn)
      return 2;
    vn = rd32(f);
    vp = malloc(vn + 1);
    if (vn && fread(vp, 1, vn, f) != vn)
      return 2;

    key = ldb_slice(kp, kn);
    val = ldb_slice(vp, vn);
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

  printf("rc=%d entries=%lu\n", rc, n);

  return rc == LDB_OK ? 0 : 1;
}
