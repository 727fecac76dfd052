#!/usr/bin/env python3
"""Generate tests/golden/merge_sweep.bin from the REFERENCE's own compactions
and its own merging iterator.

Run where make_merge_golden.py runs: beside the reference checkout, after
oracle/lcdb.mk has compiled it; never on the GPU box.  Every case of
tests/merge_sweep.py goes through tests/golden/merge_driver.c.

Repair cases (the driver's `repair` mode): the case's tables are written by
lcdb's builder (`build` mode) into an empty directory, ldb_repair puts them
at level 0, the DB is opened, the case's script runs, and
ldb_test_compact_range runs at level 0 and at level 1 with the stage dumps of
the `compact` mode.  Per step this records the input order from the stage dump
(level 0 as lcdb lists it, newest first, then the next level), the
smallest_snapshot the script implies, drop_deletions (nothing below the output
level), the kept entries' count and digest (the entries when few) and the
output file's size and SHA-256, or that lcdb wrote no file.  The files-at-level
counts of every stage are asserted: level 0 never holds four files, so no
background compaction races a dump.

Wide cases (`merge` mode): the order ldb_mergeiter_create delivers over the
case's tables.  The drop over that order is the model's, not recorded here.

Nothing recorded was computed by the code under test.  Nothing is written
unless tools/sim_merge.py reproduces every step (and tools/sim_table_split.py
every output file), drop_flags equals drop_serial, and every repair case has a
witness for its smallest_snapshot: a step whose kept entries change when the
snapshot is one lower, and, where the script wrote above its snapshot, one
whose kept entries change when it is one higher.  Without a write above the
snapshot it equals the last sequence, no parsable entry lies above it, and
nothing can depend on the higher value.

Usage: python tests/golden/make_merge_sweep_golden.py
"""
from __future__ import annotations

import hashlib
import os
import shutil
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import merge_sweep as sweep  # noqa: E402
import sim_merge  # noqa: E402
import sim_table_split  # noqa: E402
from make_merge_golden import (blob, build_table, compile_driver, parse_entries, stage,  # noqa: E402
                               table_entries)
from merge_sweep_golden_io import PATH, RECORD_MAX, Record, Step, digest, write  # noqa: E402


def write_ops(path: str, ops) -> None:
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(ops)))
        for op in ops:
            if op[0] == "p":
                f.write(struct.pack("<I", 0) + blob(op[1]) + blob(op[2]))
            elif op[0] == "d":
                f.write(struct.pack("<I", 1) + blob(op[1]))
            else:
                f.write(struct.pack("<I", 2 if op[0] == "f" else 3))


def kept_at(runs, snapshot: int, dd: int):
    return sim_merge.merge(runs, True, True, snapshot, bool(dd))[0]


def run_repair_case(driver: str, tmp: str, c) -> Record:
    src = sweep.sources(c)
    _, smallest, last = sweep.script(c)
    r = Record(c.name, c.kind, [(n, len(es), digest(es)) for n, es in sorted(src.items())])
    db, sp, od = (os.path.join(tmp, n) for n in ("db", "script", "out"))
    os.makedirs(db)
    os.makedirs(od)
    for i, t in enumerate(sweep.tables(c)):
        build_table(driver, tmp, os.path.join("db", "%06d.ldb" % (5 + 2 * i)), t, 1)
    os.remove(os.path.join(tmp, "case"))
    write_ops(sp, c.ops)
    subprocess.run([driver, "repair", db, sp, od], check=True, capture_output=True)
    stages = [stage(od, k) for k in range(3)]
    got = tuple(tuple(len(lv) for lv in s[0][:4]) for s in stages)
    assert got == c.levels, (c.name, got)
    assert all(not lv for s in stages for lv in s[0][4:]), c.name
    lower = upper = False
    for level, before, after in ((0, stages[0], stages[1]), (1, stages[1], stages[2])):
        nums = before[0][level] + before[0][level + 1]
        new = [n for lv in after[0] for n in lv if n not in before[1]]
        if not nums:
            assert not new, c.name
            continue
        dd = int(not any(before[0][level + 2:]))
        inputs = []
        for n in nums:
            es = table_entries(before[1][n])
            (name,) = [s for s, want in src.items() if want == es]
            inputs.append(name)
        assert len(set(inputs)) == len(inputs) and len(new) <= 1, c.name
        assert all(n not in [x for lv in after[0] for x in lv] for n in nums), c.name
        runs = [src[n] for n in inputs]
        st = Step(f"{c.name}:level{level}", inputs, smallest, dd)
        kept = table_entries(after[1][new[0]]) if new else []
        if new:
            assert after[0][level + 1] == new, c.name
            img = after[1][new[0]]
            st.out_bytes, st.out_sha256 = len(img), hashlib.sha256(img).digest()
            _, (mine,) = sim_table_split.split_serial(kept, *sweep.OPTIONS, True)
            assert mine == img, f"{st.name}: the model's file differs from lcdb's"
        st.count, st.digest = len(kept), digest(kept)
        st.entries = kept if len(kept) <= RECORD_MAX else None
        assert kept_at(runs, smallest, dd) == kept, f"{st.name}: the model keeps other entries"
        keys = [k for k, _ in sim_merge.merge(runs, True)[0]]
        assert sim_merge.drop_flags(keys, smallest, bool(dd)) == \
            sim_merge.drop_serial(keys, smallest, bool(dd)), st.name
        lo = kept_at(runs, smallest - 1, dd) != kept
        up = kept_at(runs, smallest + 1, dd) != kept
        lower, upper = lower or lo, upper or up
        print(f"  {st.name}: {'+'.join(inputs)}, snapshot {smallest:#x} of {last:#x}, "
              f"drop_deletions {dd}, {sum(len(x) for x in runs)} -> {len(kept)} entries, "
              f"{'no file' if not new else '%d bytes' % st.out_bytes}, "
              f"witness {'-1 ' if lo else ''}{'+1' if up else ''}")
        if level == 0:
            src = dict(src, o0=kept)
        r.steps.append(st)
    assert r.steps and lower, f"{c.name}: no witness one under the snapshot"
    assert upper or last == smallest, f"{c.name}: no witness one over the snapshot"
    return r


def run_wide_case(driver: str, tmp: str, c) -> Record:
    ts = sweep.tables(c)
    r = Record(c.name, c.kind, [("t%d" % i, len(t), digest(t)) for i, t in enumerate(ts)])
    paths = [build_table(driver, tmp, "t%d.ldb" % i, t, 1) for i, t in enumerate(ts)]
    op = os.path.join(tmp, "out")
    subprocess.run([driver, "merge", "1", op, *paths], check=True, capture_output=True)
    status, got = parse_entries(open(op, "rb").read())
    assert status == 0 and len(got) == sum(len(t) for t in ts), c.name
    r.count, r.digest = len(got), digest(got)
    r.entries = got if len(got) <= RECORD_MAX else None
    mine, order, _ = sim_merge.merge(ts, True)
    assert mine == got and order == sim_merge.merge_serial(ts, True), c.name
    keys = [k for k, _ in got]
    for snap in c.snapshots:
        for dd in (False, True):
            assert sim_merge.drop_flags(keys, snap, dd) == sim_merge.drop_serial(keys, snap, dd)
    print(f"  {c.name}: {len(ts)} tables, {len(got)} entries")
    return r


def main() -> None:
    records = []
    with tempfile.TemporaryDirectory() as top:
        driver = compile_driver(top)
        for c in sweep.all_cases():
            tmp = os.path.join(top, "case")
            os.makedirs(tmp)
            records.append((run_repair_case if c.kind == "repair" else run_wide_case)(driver, tmp, c))
            shutil.rmtree(tmp)
    size = write(PATH, records)
    steps = sum(len(r.steps) for r in records)
    print(f"{PATH}: {len(records)} cases, {steps} compaction steps, {size} bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
