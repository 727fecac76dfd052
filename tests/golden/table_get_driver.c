/*
 * table_get_driver.c -- point lookups in one SSTable by lcdb's own table
 * reader (src/table/table.c, unchanged): ldb_table_open, then
 * ldb_table_internal_get per query.  Compiled by
 * tests/golden/make_get_golden.py against the reference's headers and
 * oracle/_ref/lcdb/liblcdb_core.a + refsnappy.o; test infrastructure only,
 * never linked into the product.
 *
 * Case file (little-endian u32s): internal_keys, bits_per_key,
 * paranoid_checks, verify_checksums, n; then per query: key length, key.
 * internal_keys = 1: the table uses the DB's comparator and filter policy
 * (dbformat.c:206-345), as db_impl.c:455-460 sets them up.
 *
 * Output: i32 rc of ldb_table_open; if it is LDB_OK, per query: i32 rc,
 * u8 called (handle_result ran), u32 key length, key, u32 value length,
 * value (both as handle_result got them).
 *
 * usage: table_get_driver TABLE.ldb CASE OUT
 *        table_get_driver --time TABLE.ldb CASE REPS
 *          (the same lookups REPS times over; prints the best pass's
 *           nanoseconds per lookup)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "dbformat.h"
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

typedef struct result_s {
  int called;
  unsigned char *key;
  size_t key_len;
  unsigned char *val;
  size_t val_len;
  unsigned long sink;
} result_t;

static void
save_result(void *arg, const ldb_slice_t *k, const ldb_slice_t *v) {
  result_t *r = (result_t *)arg;

  r->called = 1;
  r->key_len = k->size;
  r->val_len = v->size;
  r->key = malloc(k->size + 1);
  r->val = malloc(v->size + 1);

  memcpy(r->key, k->data, k->size);
  memcpy(r->val, v->data, v->size);
}

static void
touch_result(void *arg, const ldb_slice_t *k, const ldb_slice_t *v) {
  result_t *r = (result_t *)arg;

  r->called = 1;
  r->sink += k->size + v->size + (v->size ? v->data[v->size - 1] : 0);
}

int
main(int argc, char **argv) {
  ldb_comparator_t icmp;
  ldb_bloom_t user_bloom, ifp;
  ldb_dbopt_t options;
  ldb_readopt_t ropt;
  ldb_rfile_t *file;
  ldb_table_t *table;
  unsigned long internal, bits, n, i, reps = 0;
  unsigned char **keys;
  size_t *lens;
  uint64_t size;
  int timing, rc;
  FILE *f, *out = NULL;

  timing = argc == 5 && strcmp(argv[1], "--time") == 0;

  if (!timing && argc != 4) {
    fprintf(stderr, "usage: %s TABLE.ldb CASE OUT | --time TABLE.ldb CASE REPS\n",
            argv[0]);
    return 2;
  }

  if (timing) {
    argv++;
    reps = strtoul(argv[3], NULL, 10);
  }

  if ((f = fopen(argv[2], "rb")) == NULL) {
    fprintf(stderr, "%s: cannot open\n", argv[2]);
    return 2;
  }

  internal = rd32(f);
  bits = rd32(f);

  options = *ldb_dbopt_default;
  options.paranoid_checks = (int)rd32(f);
  options.block_cache = NULL;

  ropt = *ldb_readopt_default;
  ropt.verify_checksums = (int)rd32(f);

  options.comparator = ldb_bytewise_comparator;
  if (internal) {
    ldb_ikc_init(&icmp, ldb_bytewise_comparator);
    options.comparator = &icmp;
  }

  options.filter_policy = NULL;
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
    unsigned long r, hits = 0, sink = 0;

    if (rc != LDB_OK) {
      fprintf(stderr, "open: %s\n", ldb_strerror(rc));
      return 1;
    }

    for (r = 0; r < reps; r++) {
      struct timespec t0, t1;
      double ns;

      clock_gettime(CLOCK_MONOTONIC, &t0);

      for (i = 0; i < n; i++) {
        ldb_slice_t k = ldb_slice(keys[i], lens[i]);
        result_t res;

        res.called = 0;
        res.sink = 0;
        ldb_table_internal_get(table, &ropt, &k, &res, touch_result);
        hits += res.called;
        sink += res.sink;
      }

      clock_gettime(CLOCK_MONOTONIC, &t1);

      ns = (t1.tv_sec - t0.tv_sec) * 1e9 + (t1.tv_nsec - t0.tv_nsec);
      if (r == 0 || ns < best)
        best = ns;
    }

    printf("lookups=%lu reps=%lu hits=%lu sink=%lu ns_per_lookup=%.1f\n", n, reps,
           hits, sink, n ? best / n : 0.0);

    ldb_table_destroy(table);
    ldb_rfile_destroy(file);
    return 0;
  }

  if ((out = fopen(argv[3], "wb")) == NULL)
    return 2;

  wr32(out, (unsigned long)rc);

  if (rc == LDB_OK) {
    for (i = 0; i < n; i++) {
      ldb_slice_t k = ldb_slice(keys[i], lens[i]);
      result_t res;
      int grc;

      memset(&res, 0, sizeof(res));
      grc = ldb_table_internal_get(table, &ropt, &k, &res, save_result);

      wr32(out, (unsigned long)grc);
      fputc(res.called, out);
      wr32(out, (unsigned long)res.key_len);
      if (res.key_len)
        fwrite(res.key, 1, res.key_len, out);
      wr32(out, (unsigned long)res.val_len);
      if (res.val_len)
        fwrite(res.val, 1, res.val_len, out);

      free(res.key);
      free(res.val);
    }

    ldb_table_destroy(table);
  }

  ldb_rfile_destroy(file);
  fclose(out);

  printf("open=%d queries=%lu\n", rc, n);

  return 0;
}
