#!/usr/bin/env python3
"""Generate tests/golden/compact_split.bin from the REFERENCE table builder and
one of the REFERENCE's own compactions.

Run where make_merge_golden.py runs: beside the reference checkout, after
oracle/lcdb.mk has compiled it (oracle/_ref/lcdb/liblcdb_core.a, refsnappy.o);
never on the GPU box.  Compiles tests/golden/split_driver.c against the
reference's headers.

Split cases: the driver feeds a case's entries to lcdb's ldb_tablegen_* the
way ldb_do_compaction_work does (db_impl.c:1399-1425) with the case's
max_output_file_size, which the DB itself clips to 1 MiB and more
(db_impl.c:341); every output file is read back here.

The compaction: the driver opens a fresh DB with max_file_size = 1 MiB and no
compression, writes split_golden_io.compact_ops' level-0 files (the first
through a reopen, the others through memtable flushes, so that all of them
stay in level 0 and levels 1 and 2 are empty: no grandparents, so
ldb_compaction_should_stop_before never fires) and runs
ldb_test_compact_range at level 0.  Inputs and outputs are copied out.

Nothing recorded was computed by the code under test;
tools/sim_table_split.py must reproduce every recorded file before the
fixture is written.

Usage: python tests/golden/make_split_golden.py
"""
from __future__ import annotations

import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import oracle  # noqa: E402
import sim_merge  # noqa: E402
import sim_table_split as sim  # noqa: E402
import table_golden_io  # noqa: E402
from make_get_golden import CFLAGS, LCDB  # noqa: E402
from sim_block_cut import serial_blocks  # noqa: E402
from sim_table_scan import ST_OK, Table, scan  # noqa: E402
from split_golden_io import (NO_SPLIT, PATH, CompactCase, SplitCase, compact_inputs,  # noqa: E402
                             compact_ops, digest, gen_entries, out_file, tag, write)

IMAGES_MAX = 4096                                   # a case's images are kept up to this total


def compile_driver(tmp: str) -> str:
    driver = os.path.join(tmp, "split_driver")
    subprocess.run(["gcc", *CFLAGS, os.path.join(HERE, "split_driver.c"),
                    os.path.join(LCDB, "refsnappy.o"), os.path.join(LCDB, "liblcdb_core.a"),
                    "-lpthread", "-o", driver], check=True)
    return driver


def blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


# ---- split cases -----------------------------------------------------------

def framed(entries, block_size, restart_interval, compression):
    """(start, end) of every data block of one cut framed from offset 0."""
    _, blocks = serial_blocks(entries, block_size, restart_interval)
    _, hoff, hsize, _ = oracle.table_write_blocks(blocks, compression, 0)
    return [int(x) for x in hoff], [int(o) + int(s) + 5 for o, s in zip(hoff, hsize)]


def file_blocks(start, end, max_size):
    """[(first block, block after the last)] of the files."""
    out, s = [], 0
    while s < len(start):
        b = s
        while b + 1 < len(start) and end[b] - start[s] < max_size:
            b += 1
        out.append((s, b + 1))
        s = b + 1
    return out


def split_cases(sets):
    out = []

    def case(name, source, bs, R, comp, bits, internal, mx, own=None):
        out.append(SplitCase(name, source, bs, R, comp, bits, internal, mx, own=own or []))

    # About 300 entries of 16 + 32 bytes in 256-byte blocks.
    gen = "gen:300:3:0"
    e = gen_entries(300, 3, 0)
    start, end = framed(e, 256, 16, 0)
    case("gen300_1024", gen, 256, 16, 0, 0, 0, 1024)
    case("gen300_1024_snappy", gen, 256, 16, 1, 0, 0, 1024)
    case("gen300_every_block", gen, 256, 16, 0, 0, 0, 1)
    case("gen300_one_file", gen, 256, 16, 0, 0, 0, NO_SPLIT)
    # max_output_file_size exactly the first file's data bytes (the >= is
    # inclusive: the same first file), and one more (one more block).
    s0, e0 = file_blocks(start, end, 1024)[0]
    exact = end[e0 - 1] - start[s0]
    assert file_blocks(start, end, exact)[0] == (s0, e0)
    assert file_blocks(start, end, exact + 1)[0] == (s0, e0 + 1)
    case("gen300_exact", gen, 256, 16, 0, 0, 0, exact)
    case("gen300_exact_plus_1", gen, 256, 16, 0, 0, 0, exact + 1)
    # The last file closed by its last entry: no empty file behind it.
    for mx in range(900, 4000):
        fb = file_blocks(start, end, mx)
        s, b = fb[-1]
        if len(fb) > 2 and end[b - 1] - start[s] >= mx:
            case("gen300_ends_with_last_block", gen, 256, 16, 0, 0, 0, mx)
            break
    else:
        raise AssertionError("no size closes the last file with the last block")
    # Filters that span several 2 KiB ranges per file.
    case("gen300_filter", gen, 256, 16, 0, 10, 0, 6000)
    case("gen300_internal_filter_snappy", "gen:300:3:1", 256, 16, 1, 10, 1, 5000)
    # Internal keys, every entry the last of its file: successors that do not
    # shorten (all 0xff, empty, one byte) and that do.
    users = [b"", b"\x00", b"a", b"ab\xff", b"abc", b"b\xff\xff\xff", b"\xfe", b"\xff",
             b"\xff\x00", b"\xff\x01z", b"\xff\xff", b"\xff\xff\xff\xff", b"\xff\xff\xff\xff\x41"]
    own = [(u + tag(50 + i, i % 2), b"v%02d" % i) for i, u in enumerate(sorted(users))]
    case("successors_internal_every_entry", "", 1, 16, 0, 0, 1, 1, own)
    case("successors_internal_filter", "", 1, 16, 1, 10, 1, 60, own)
    bytewise = [(u, b"v%02d" % i) for i, u in enumerate(sorted(users))]
    case("successors_bytewise_every_entry", "", 1, 16, 0, 10, 0, 1, bytewise)
    # A file-last user key of 0xff bytes among longer files, and one that shortens.
    ff = [(b"\xfe" * 6 + b"%02d" % i + tag(9, 1), b"y" * 40) for i in range(12)] + \
         [(b"\xff" * 6 + tag(9, 1), b"x" * 40)]
    case("last_user_key_all_ff", "", 200, 16, 0, 0, 1, 400, ff)
    # Entry sets lcdb's builder has already written whole.
    for name, mx in (("fill256", 1024), ("fill256", 1), ("fill256_internal", 2000),
                     ("fill4096", 4096), ("fill4096_internal", 6000), ("own_block", 100),
                     ("own_block_internal", 1), ("separators", 1), ("separators_internal", 1),
                     ("separators_internal", 150), ("count17", 1), ("count1", 1),
                     ("varint", 70000)):
        s = next(x for x in sets if x.name == name)
        for v in s.variants:
            case(f"{name}_{v.block_size}_{v.restart_interval}_{v.compression}_{v.bits_per_key}_{mx}",
                 name, v.block_size, v.restart_interval, v.compression, v.bits_per_key, v.internal,
                 mx)
    return out


def run_split_case(driver, tmp, c: SplitCase, sets) -> None:
    es = c.entries(sets)
    c.count, c.digest = len(es), digest(es)
    od = os.path.join(tmp, "split_" + c.name)
    os.makedirs(od)
    cp = os.path.join(od, "case")
    with open(cp, "wb") as f:
        f.write(struct.pack("<8I", c.block_size, c.restart_interval, c.compression, c.bits_per_key,
                            c.internal, c.max_file_size & 0xffffffff, c.max_file_size >> 32,
                            len(es)))
        for k, v in es:
            f.write(blob(k) + blob(v))
    subprocess.run([driver, "split", cp, od], check=True)
    rows = [[int(x) for x in ln.split()] for ln in open(os.path.join(od, "split.txt"))]
    images = [open(os.path.join(od, "%06d.ldb" % r[0]), "rb").read() for r in rows]
    keep = sum(len(i) for i in images) <= IMAGES_MAX
    at = 0
    for (idx, n, size), img in zip(rows, images):
        assert size == len(img) and n > 0, c.name
        c.files.append(out_file(es[at:at + n], img, keep))
        at += n
    assert at == len(es), c.name
    first, mine = sim.split_serial(es, c.block_size, c.restart_interval, c.compression,
                                   c.bits_per_key, bool(c.internal), c.max_file_size)
    assert mine == images, c.name
    assert first == sim.split_blocks(es, c.block_size, c.restart_interval, c.compression,
                                     c.max_file_size), c.name
    print(f"  {c.name}: {len(es)} entries -> {len(images)} files"
          f"{' (images kept)' if keep else ''}")


# ---- the compaction --------------------------------------------------------

L0_FILES, USER_KEYS = 3, 20000     # under the level-0 compaction trigger of 4 files


def levels_of(text: str):
    """[[(file number, bytes)] per level] of the "leveldb.sstables" property."""
    levels, level = [[] for _ in range(7)], None
    for ln in text.splitlines():
        m = re.match(r"--- level (\d+) ---", ln)
        if m:
            level = int(m.group(1))
            continue
        m = re.match(r" (\d+):(\d+)\[", ln)
        if m:
            levels[level].append((int(m.group(1)), int(m.group(2))))
    return levels


def table_entries(img: bytes):
    st, es = scan(Table(img, internal=True, filter_name=None))
    assert st == ST_OK
    return es


def run_compaction(driver, tmp) -> CompactCase:
    db, sp, od = (os.path.join(tmp, n) for n in ("db", "script", "out"))
    groups = compact_ops(L0_FILES, USER_KEYS)
    ops = []
    for j, grp in enumerate(groups):
        ops += grp + [("r",) if j == 0 else ("f",)]
    with open(sp, "wb") as f:
        f.write(struct.pack("<I", len(ops)))
        for op in ops:
            if op[0] == "p":
                f.write(struct.pack("<I", 0) + blob(op[1]) + blob(op[2]))
            elif op[0] == "d":
                f.write(struct.pack("<I", 1) + blob(op[1]))
            else:
                f.write(struct.pack("<I", 2 if op[0] == "f" else 4))
    os.makedirs(od)
    subprocess.run([driver, "compact", db, sp, od], check=True, capture_output=True)
    before = levels_of(open(os.path.join(od, "stage0.txt")).read())
    after = levels_of(open(os.path.join(od, "stage1.txt")).read())
    # All inputs in level 0 and nothing below: no grandparents, so
    # should_stop_before cannot fire, and level 1 is the base level for every key.
    assert [len(lv) for lv in before] == [L0_FILES, 0, 0, 0, 0, 0, 0], before
    assert [len(lv) for lv in after] == [0, 3, 0, 0, 0, 0, 0], after
    inputs, last = compact_inputs(L0_FILES, USER_KEYS)
    c = CompactCase(L0_FILES, USER_KEYS, last, 1, 4096, 16, 0, 0, 1 << 20)
    total = 0
    for (num, size), es in zip(sorted(before[0]), inputs):       # file numbers grow with age
        img = open(os.path.join(od, "stage0", "%06d.ldb" % num), "rb").read()
        assert len(img) == size and table_entries(img) == es, num
        # What the test rebuilds each input with must be this table.
        assert sim.split_serial(es, 4096, 16, 0, 0, True)[1] == [img], num
        c.inputs.append((len(es), hashlib.sha256(img).digest()))
        total += len(img)
    kept, _, dropped = sim_merge.merge(list(reversed(inputs)), True, True, last, True)
    first, mine = sim.split_serial(kept, 4096, 16, 0, 0, True, 1 << 20)
    outs = [open(os.path.join(od, "stage1", "%06d.ldb" % num), "rb").read()
            for num, _ in sorted(after[1])]
    assert mine == outs, "the model's files differ from lcdb's"
    for f, img in enumerate(outs):
        assert table_entries(img) == kept[first[f]:first[f + 1]]
        c.files.append(out_file(kept[first[f]:first[f + 1]], img, False))
    print(f"  compaction: {L0_FILES} level-0 files of {total} bytes, {sum(n for n, _ in c.inputs)}"
          f" entries -> {len(kept)} kept ({dropped} dropped) in {len(outs)} files of "
          f"{[len(i) for i in outs]} bytes")
    return c


def main() -> None:
    sets = table_golden_io.read()
    cases = split_cases(sets)
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        for c in cases:
            run_split_case(driver, tmp, c, sets)
        compact = run_compaction(driver, tmp)
    size = write(PATH, cases, compact)
    print(f"{PATH}: {len(cases)} split cases, 1 compaction, {size} bytes")
    assert size < 256 * 1024


if __name__ == "__main__":
    main()
