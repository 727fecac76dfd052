#!/usr/bin/env python3
"""Generate tests/golden/read_sweep.bin from the REFERENCE table reader.

Run where make_get_golden.py runs: beside the reference checkout, after
oracle/lcdb.mk has compiled it; never on the GPU box.  Every table of
tests/read_sweep.py is written to a temporary file and read by lcdb itself,
through the unchanged tests/golden/table_get_driver.c (ldb_table_open +
ldb_table_internal_get per target) and table_scan_driver.c (ldb_tableiter
seek + next to the end per start).

The bytes of a sweep table are the CPU model's image, used only where its
length and SHA-256 are what lcdb's builder wrote (build_sweep.bin).  The
tables of the `versions` family are built here by lcdb's builder
(table_golden_driver.c, as make_table_golden.py runs it); their size and
SHA-256 are recorded and the model's image must equal them.

Recorded per target: lcdb's return code, whether handle_result was called,
and the ordinal of the entry whose key and value bytes it was handed (asserted
here).  A filtered table is read a second time without a filter policy: a
target that is called only then was refused by the filter.  Recorded per
start: the final status, the count, and the ordinal of the first entry; the
delivered list is asserted to be entries[ordinal:] by its SHA-256.  Nothing
recorded is computed by the code under test or by the model.

The `versions` entry set (read_sweep._versions), all internal keys:
  - the empty user key; user keys of 7, 8 and 9 bytes and their 00 successors;
  - for p in 0..6 a chain `eq<p>` of 22 values and a chain `mix<p>` of 12
    deletions and values whose sequences are (j << 8p) | low with j falling:
    neighbours share the type byte (where equal) and p sequence bytes;
  - chains of 2 to 40 versions with random sequences below 2^8 .. 2^56;
  - `edges`: sequences at merge_sweep.S_EDGES, at 2^56 - 1, and one below each;
  - `cont<n>`: a user key, then that user key and the leading n bytes of its
    last tag as the next user key, n in 1..8;
  - `long`: 300 versions, which no block of 4096 bytes holds.

The conditions asserted on what lcdb returned, and what it gave (printed by
the last run of this recipe):
    tables 118, all opened; targets 54 878; starts 1 329
    refused by the filter                                  >= 1000:  3 356
    between-blocks misses (not called, OK, a later entry;
      filter refusals not counted)                         >= 1000:  1 414
    finds whose entry shares 1 byte of its tag             >=  200:  1 675
    finds whose entry shares 2, 3, .. 7 bytes of its tag   >=   20 each:
                                                           68, 58, 54, 87, 46, 58
    internal-key targets under 8 bytes                     >=   30:  558

Usage: python tests/golden/make_read_sweep_golden.py
"""
from __future__ import annotations

import hashlib
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import read_sweep as rs  # noqa: E402
import make_get_golden  # noqa: E402
import make_scan_golden  # noqa: E402
import make_table_golden  # noqa: E402
import sim_table_get as sim  # noqa: E402
import sim_table_scan  # noqa: E402
import table_get_golden_io  # noqa: E402
import table_io  # noqa: E402
import table_scan_golden_io  # noqa: E402
from merge_golden_io import digest  # noqa: E402
from read_sweep_golden_io import CALLED, NONE, PATH, REFUSED, Record, write  # noqa: E402


def lcdb_gets(driver, tmp, img, t, bits, keys):
    c = table_get_golden_io.Case(t.name, "", 0, [], t.internal, bits, 0, 1)
    make_get_golden.run_driver(driver, tmp, img, c, keys)
    return c


def main() -> None:
    tables = rs.tables()
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        get_driver = make_get_golden.compile_driver(tmp)
        scan_driver = make_scan_golden.compile_driver(tmp)
        gen_driver = os.path.join(tmp, "table_golden_driver")
        make_get_golden.subprocess.run(
            ["gcc", *make_get_golden.CFLAGS, os.path.join(HERE, "table_golden_driver.c"),
             os.path.join(make_get_golden.LCDB, "refsnappy.o"),
             os.path.join(make_get_golden.LCDB, "liblcdb_core.a"), "-lpthread", "-o", gen_driver],
            check=True)
        for t in tables:
            es = rs.entries(t)
            r = Record(t.name, t.case, t.file)
            if t.versions:
                img = make_table_golden.run_driver(gen_driver, tmp, es, t.block_size,
                                                   t.restart_interval, t.compression,
                                                   t.bits_per_key, t.internal)
                r.count, r.digest = len(es), digest(es)
                r.size, r.sha = len(img), hashlib.sha256(img).digest()
                assert rs.image(t, (r.size, r.sha)) == img, f"{t.name}: the model's file differs"
            else:
                img = rs.image(t, rs.sweep_pin(t))
            ordinal = {k: i for i, (k, _) in enumerate(es)}
            keys = rs.targets(t)
            c = lcdb_gets(get_driver, tmp, img, t, t.bits_per_key, keys)
            plain = lcdb_gets(get_driver, tmp, img, t, 0, keys) if t.bits_per_key else c
            r.open_rc = c.open_rc
            assert c.open_rc == table_io.LDB_OK == plain.open_rc, t.name
            for k, a, b in zip(keys, c.records, plain.records):
                if a.called:
                    o = ordinal[a.found_key]
                    assert es[o] == (a.found_key, a.found_value), (t.name, k)
                    assert (a.rc, a.found_key, a.found_value) == (b.rc, b.found_key, b.found_value)
                else:
                    assert a.found_key == b"" == a.found_value
                r.rc.append(a.rc)
                r.flags.append(CALLED if a.called else (REFUSED if b.called else 0))
                r.ordinal.append(o if a.called else NONE)
            sc = table_scan_golden_io.Case(t.name, "", 0, [], t.internal, t.bits_per_key, 0, 1)
            make_scan_golden.run_driver(scan_driver, tmp, img, sc, rs.starts(t))
            assert sc.open_rc == table_io.LDB_OK, t.name
            full = sc.runs[0]
            assert (full.rc, full.count, full.digest) == (0, len(es), sim_table_scan.digest(es))
            for run in sc.runs[1:]:
                o = len(es) - run.count
                assert run.digest == sim_table_scan.digest(es[o:]), (t.name, run.start)
                r.starts.append((run.rc, run.count, o))
            records.append(r)
            print(f"  {t.name}: {len(es)} entries, {len(keys)} targets, "
                  f"{sum(f & CALLED for f in r.flags)} called, {len(r.starts)} starts")
    n = rs.conditions(tables, records)
    print(f"tables {len(records)}, targets {sum(len(r.rc) for r in records)}, "
          f"starts {sum(len(r.starts) for r in records)}")
    print(f"refused by the filter {n['refused']}, between-blocks misses {n['between']}, "
          f"short internal targets {n['short']}")
    print("finds by tag bytes shared: " +
          ", ".join(f"{p}: {n['shared', p]}" for p in range(9)))
    rs.check_conditions(n)
    size = write(PATH, records)
    print(f"{PATH}: {size} bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
