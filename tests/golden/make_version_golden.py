#!/usr/bin/env python3
"""Generate tests/golden/compact_version.bin from the REFERENCE's compaction
loop and one of the REFERENCE's own compactions over a populated level 2.

Run where make_split_golden.py runs: beside the reference checkout, after
oracle/lcdb.mk has compiled it (oracle/_ref/lcdb/liblcdb_core.a, refsnappy.o);
never on the GPU box.  Compiles tests/golden/version_driver.c against the
reference's headers.

Loop cases: the driver runs the body of ldb_do_compaction_work's loop
(db_impl.c:1352-1425) around lcdb's own ldb_compaction_should_stop_before,
ldb_compaction_is_base_level_for_key, ldb_pkey_import and ldb_tablegen_* over
a case's merged entries, with a hand-assembled compaction whose version holds
the case's levels.  Limits of a few hundred bytes are reachable only there.

The compaction: a fresh DB with max_file_size = 1 MiB and no compression.
Fifteen memtable flushes of about 1 MiB each, over disjoint key ranges with
gaps between them, land in level 2 (pick_level_for_memtable_output); a sparse
flush across six of them lands in level 1, a sparse flush across thirteen
stays in level 0, and ldb_test_compact_range at level 0 merges the two over
level 2.  Level 2 enters the fixture as (smallest, largest, size) only.

The recipe asserts what the recorded compaction must show, that the loop mode
fed the same inputs and levels writes the same files, and that
tools/sim_compact_version.py reproduces every recorded file and flag, before
the fixture is written.  Nothing recorded was computed by the code under test.

Usage: python tests/golden/make_version_golden.py
"""
from __future__ import annotations

import os
import random
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

import sim_compact_version as sim  # noqa: E402
import sim_merge  # noqa: E402
from compact_version_golden_io import DROP, PATH, STOP, Compaction, LoopCase, out_file, write  # noqa: E402
from make_get_golden import CFLAGS, LCDB  # noqa: E402
from sim_block_cut import serial_blocks  # noqa: E402
from sim_table_scan import ST_OK, Table, scan  # noqa: E402

IMAGES_MAX = 4096                                   # a case's images are kept up to this total
BIG = 1 << 40                                       # a snapshot above every sequence


def compile_driver(tmp: str) -> str:
    driver = os.path.join(tmp, "version_driver")
    subprocess.run(["gcc", *CFLAGS, os.path.join(HERE, "version_driver.c"),
                    os.path.join(LCDB, "refsnappy.o"), os.path.join(LCDB, "liblcdb_core.a"),
                    "-lpthread", "-o", driver], check=True)
    return driver


def blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


def ikey(user: bytes, seq: int, typ: int = 1) -> bytes:
    return user + struct.pack("<Q", (seq << 8) | typ)


def user(i: int) -> bytes:
    return b"u%07d" % i


# ---- loop cases --------------------------------------------------------------

def point_files(entries, at, size=1):
    """Level + 2 files that make should_stop_before pass one file at each
    merged position in `at` (> 0): a file whose smallest and largest key is the
    key before that position.  The key itself equals no largest."""
    return [(entries[t - 1][0], entries[t - 1][0], size) for t in sorted(at)]


def spread(rng, n_entries: int, n_files: int, deletions: bool = True, odd_types: bool = False):
    """n_entries merged entries over distinct and repeated user keys, and
    n_files disjoint level files with gaps over the same key space."""
    entries, i = [], 0
    while len(entries) < n_entries:
        i += rng.randrange(1, 4)
        versions = rng.choice([1, 1, 1, 2, 3])
        seqs = sorted(rng.sample(range(1, 200), versions), reverse=True)
        for s in seqs:
            typ = 1
            if deletions and rng.random() < 0.25:
                typ = 0
            if odd_types and rng.random() < 0.1:
                typ = rng.choice([2, 7, 255])
            if len(entries) < n_entries:
                entries.append((ikey(user(i), s, typ), b"v%05d" % rng.randrange(100000) *
                                rng.choice([1, 1, 4])))
    entries.sort(key=sim_merge.sort_key(True))
    top = i + 4
    # Disjoint in user keys up to a user key shared across a boundary, largest
    # strictly increasing.
    cuts = sorted(rng.sample(range(max(top, 2 * n_files + 2)), 2 * n_files))
    files = []
    for f in range(n_files):
        lo = ikey(user(cuts[2 * f]), rng.randrange(100, 200), 1)
        if files and rng.random() < 0.15:
            lo = ikey(files[-1][1][:-8], 5, 1)      # behind the largest key before it
        files.append((lo, ikey(user(cuts[2 * f + 1]), rng.randrange(10, 100), rng.randrange(2)),
                      rng.choice([0, 1, 40, 100, 300, 1000])))
    return entries, files


def loop_cases():
    out = []

    def case(name, entries, levels, target, snapshot=BIG, bs=256, R=16, comp=0, bits=0,
             mx=1 << 30):
        out.append(LoopCase(name, bs, R, comp, bits, mx, target, snapshot, levels=levels,
                            entries=entries))

    # Level-2 list lengths: 0, 1, 2, 65 and 300 files (300: past a 256-lane workgroup).
    for nf in (0, 1, 2, 65, 300):
        rng = random.Random(1000 + nf)
        es, files = spread(rng, 700, nf)
        case(f"files_{nf}", es, [files], 30, snapshot=120)
    # Limit edges.  Limit 1000: what the first key passes is free; 400 + 600 is
    # the limit exactly (no stop); one byte more stops; then again 1000 does
    # not and one byte more does.
    es = [(ikey(user(10 * i), 5), b"x" * 20) for i in range(12)]
    files = [(ikey(b"a", 9), ikey(b"b", 1), 5000)] + \
        [(es[t][0], es[t][0], s) for t, s in ((2, 400), (3, 600), (4, 1), (6, 1000), (8, 1))]
    case("limit_exact", es, [files], 100)
    # Limit 0: every passed file of a size above 0 stops, but not at the first key.
    es = [(ikey(user(10 * i + 10), 5), b"y" * 20) for i in range(10)]
    files = [(ikey(user(1), 9), ikey(user(2), 1), 7)] + \
        [(es[t][0], es[t][0], s) for t, s in ((0, 9), (1, 1), (3, 0), (4, 3), (7, 1))]
    case("limit_zero", es, [files], 0)
    # Several files passed by one key: G jumps by more than 1 and the base moves past nxt.
    rng = random.Random(77)
    es = [(ikey(user(100 * i), 5), b"z" * 10) for i in range(40)]
    files = [(ikey(user(10 * j), 9), ikey(user(10 * j + 3), 1), rng.choice([1, 30, 200]))
             for j in range(1, 390)]
    case("many_files_per_key", es, [files], 40)
    # Stops on dropped keys (limit 0, snapshot above everything: rule (A) drops
    # every older version).  A file's largest between two versions of one user
    # key is passed by the older one; a key equal to a largest does not pass it.
    a, b, c, d = user(1), user(2), user(3), user(4)
    es = [(ikey(a, 9), b"a9"), (ikey(a, 7), b"a7"), (ikey(a, 5), b"a5"), (ikey(a, 3), b"a3"),
          (ikey(b, 8), b"b8"), (ikey(c, 8), b"c8"), (ikey(c, 6), b"c6"), (ikey(d, 4), b"d4"),
          (ikey(d, 2), b"d2"), (ikey(d, 1), b"d1")]
    files = [(ikey(a, 8), ikey(a, 7), 1),          # (a,7) equals it: passed by (a,5), dropped
             (ikey(a, 4), ikey(a, 4), 1),          # passed by (a,3), dropped: same span, one start
             (ikey(c, 9), ikey(c, 7), 1),          # passed by (c,6), dropped: the start moves to d
             (ikey(d, 3), ikey(d, 3), 1),          # passed by (d,2): nothing kept behind it
             (ikey(d, 2), ikey(d, 2), 1)]          # passed by (d,1)
    case("stops_on_dropped", es, [files], 0)
    case("stop_at_second_key", es[:5], [[(es[0][0], es[0][0], 3)]], 0)
    # A stop directly behind a size-driven close: every entry fills its block
    # and every block its file.
    es = [(ikey(user(i), 5), b"w" * 30) for i in range(9)]
    case("stop_behind_size_close", es, [point_files(es, [1, 4, 5, 8])], 0, bs=1, mx=1)
    # Type bytes above 1: kept, ordered by the raw tag, and they pass files.
    rng = random.Random(5)
    es, files = spread(rng, 300, 30, odd_types=True)
    case("odd_types", es, [files], 10, snapshot=150)
    # Base level edges.
    lv2 = [(ikey(b"c0", 50), ikey(b"f0", 3), 10), (ikey(b"h0", 50), ikey(b"m", 9), 10),
           (ikey(b"m", 3), ikey(b"p0", 1), 10)]            # m: shared by two files
    lv4 = [(ikey(b"r0", 9), ikey(b"r0", 2), 5)]
    dels = [b"c", b"c0", b"c00", b"f", b"f0", b"f0\x00", b"g", b"h0", b"m", b"m\x00", b"p0",
            b"p1", b"q", b"r0", b"r0\x00", b"s"]
    es = [(ikey(u, 7, 0), b"") for u in dels] + \
        [(ikey(b"z", 20, 1), b"new"), (ikey(b"z", 10, 0), b"")]   # hidden by (A) whatever base says
    es.sort(key=sim_merge.sort_key(True))
    case("base_one_level", es, [lv2], 1000, snapshot=100)
    case("base_five_levels", es, [lv2, [], lv4, [(ikey(b"z", 99), ikey(b"zz", 1), 1)],
                                  [(ikey(b"", 9), ikey(b"a", 1), 1)]], 1000, snapshot=100)
    case("base_snapshot_below", es, [lv2], 1000, snapshot=6)
    # Forced cut edges: a forced start at a size-driven block start, one entry
    # before it and one behind it; two on consecutive entries.
    es = [(ikey(user(i), 5), (b"%06d" % i) * 5) for i in range(120)]
    bf, _ = serial_blocks(es, 256, 16)
    s = bf[2]
    assert bf[1] + 1 < s - 1 and s + 1 < bf[3] - 1
    for name, at in (("at_block_start", [s]), ("before_block_start", [s - 1]),
                     ("behind_block_start", [s + 1]), ("consecutive", [s + 3, s + 4]),
                     ("all_three", [s - 1, s, s + 1])):
        case("forced_" + name, es, [point_files(es, at)], 0)
    at = [s - 1, s + 1, bf[4], bf[6] + 2, bf[6] + 3, 100]
    case("forced_restart_1", es, [point_files(es, at)], 0, R=1)
    case("forced_snappy", es, [point_files(es, at)], 0, comp=1)
    case("forced_filter", es, [point_files(es, at)], 0, bits=10, mx=900)
    case("forced_filter_snappy_restart_3", es, [point_files(es, at)], 0, R=3, comp=1, bits=10, mx=600)
    case("forced_every_block_a_file", es, [point_files(es, at)], 0, mx=1)
    # Entry counts: 1, 2, 255, 256, 257 and about 5000.
    for n in (1, 2, 255, 256, 257, 5000):
        rng = random.Random(3000 + n)
        es, files = spread(rng, n, 3 if n < 10 else 40)
        case(f"entries_{n}", es, [files, files[::3]], 20 if n < 5000 else 60, snapshot=120,
             bs=256 if n < 5000 else 1024, mx=1 << 30 if n < 5000 else 20000)
    return out


def run_loop(driver, tmp, c, tag="loop_"):
    """The driver on a case: (flags, images)."""
    od = os.path.join(tmp, tag + c.name)
    os.makedirs(od)
    cp = os.path.join(od, "case")
    with open(cp, "wb") as f:
        f.write(struct.pack("<4I3Q", c.block_size, c.restart_interval, c.compression,
                            c.bits_per_key, c.max_output_file_size, c.max_file_size,
                            c.smallest_snapshot))
        f.write(struct.pack("<I", len(c.levels)))
        for files in c.levels:
            f.write(struct.pack("<I", len(files)))
            for lo, hi, size in files:
                f.write(blob(lo) + blob(hi) + struct.pack("<Q", size))
        f.write(struct.pack("<I", len(c.entries)))
        for k, v in c.entries:
            f.write(blob(k) + blob(v))
    subprocess.run([driver, "loop", cp, od], check=True)
    rows = [[int(x) for x in ln.split()] for ln in open(os.path.join(od, "loop.txt"))]
    images = [open(os.path.join(od, "%06d.ldb" % r[0]), "rb").read() for r in rows]
    for (_, n, size), img in zip(rows, images):
        assert size == len(img) and n > 0, c.name
    flags = bytes(STOP * int(ln.split()[0]) | DROP * int(ln.split()[1])
                  for ln in open(os.path.join(od, "flags.txt")))
    return flags, [r[1] for r in rows], images


def check_levels(c):
    for files in c.levels:
        for j, (lo, hi, _) in enumerate(files):
            assert len(lo) >= 8 and len(hi) >= 8 and sim_merge.compare(lo, hi, True) <= 0, c.name
            if j:
                assert sim_merge.compare(files[j - 1][1], hi, True) < 0, c.name
                assert files[j - 1][1][:-8] <= lo[:-8], c.name


def record_loop(driver, tmp, c) -> None:
    check_levels(c)
    keys = [k for k, _ in c.entries]
    assert all(sim_merge.compare(keys[i], keys[i + 1], True) <= 0 for i in range(len(keys) - 1))
    c.flags, counts, images = run_loop(driver, tmp, c)
    assert len(c.flags) == len(c.entries), c.name
    kept = c.kept()
    keep = sum(len(i) for i in images) <= IMAGES_MAX
    at = 0
    for n, img in zip(counts, images):
        c.files.append(out_file(kept[at:at + n], img, keep))
        at += n
    assert at == len(kept), c.name
    # The model: its serial loop is lcdb's, its parallel formulation its serial loop.
    stops, drops = sim.loop_serial(keys, c.smallest_snapshot, c.levels, c.limit)
    assert bytes(STOP * s | DROP * d for s, d in zip(stops, drops)) == c.flags, c.name
    args = (c.smallest_snapshot, c.levels, c.limit, c.block_size, c.restart_interval,
            c.compression, c.bits_per_key, c.max_output_file_size)
    want = sim.compact_serial(c.entries, *args)
    assert want == (kept, c.file_first(), images), c.name
    assert sim.compact_parallel(c.entries, *args) == want, c.name
    print(f"  {c.name}: {len(c.entries)} entries, {sum(len(f) for f in c.levels)} level files, "
          f"{sum(1 for f in c.flags if f & STOP)} stops, {len(c.entries) - len(kept)} dropped -> "
          f"{len(images)} files{' (images kept)' if keep else ''}")


def check_cases(cases) -> None:
    """The situations the cases are there for, in lcdb's own answers."""
    by = {c.name: c for c in cases}

    def stops(c):
        return [i for i, f in enumerate(c.flags) if f & STOP]

    def drops(c):
        return [i for i, f in enumerate(c.flags) if f & DROP]

    assert stops(by["limit_exact"]) == [5, 9]
    assert stops(by["limit_zero"]) == [1, 2, 5, 8]
    c = by["stops_on_dropped"]
    assert stops(c) == [2, 3, 6, 8, 9] and drops(c) == [1, 2, 3, 6, 8, 9]
    assert c.file_first() == [0, 1, 3, 4]           # a | b c | d: no file behind the last stops
    assert stops(by["stop_at_second_key"]) == [1] and len(by["stop_at_second_key"].files) == 2
    c = by["stop_behind_size_close"]
    assert stops(c) == [1, 4, 5, 8] and [f.entries for f in c.files] == [1] * 9
    assert any(k[-8] > 1 for k, _ in by["odd_types"].entries)
    c = by["base_one_level"]
    kept_dels = {k[:-8] for k, _ in c.kept() if k[-8] == 0}
    assert kept_dels == {b"c0", b"c00", b"f", b"f0", b"h0", b"m", b"m\x00", b"p0"}, kept_dels
    c = by["base_five_levels"]
    assert {k[:-8] for k, _ in c.kept() if k[-8] == 0} == kept_dels | {b"r0"}
    assert not any(k[:-8] == b"z" and k[-8] == 0 for k, _ in c.kept())
    assert not drops(by["base_snapshot_below"])
    assert len(by["forced_consecutive"].files) == 3 and by["forced_consecutive"].files[1].entries == 1
    assert len(by["forced_at_block_start"].files) == 2
    assert any(len(f) == 300 for f in by["files_300"].levels)
    assert len(by["forced_every_block_a_file"].files) > len(by["forced_filter"].files) > 3
    many = by["many_files_per_key"]
    g = sim.passed([k for k, _ in many.entries], many.levels[0])
    assert max(b - a for a, b in zip(g, g[1:])) > 5 and stops(many)
    assert len(by["entries_5000"].files) > 3 and len(stops(by["entries_5000"])) > 3


# ---- the compaction ------------------------------------------------------------

L2_FILES, L2_KEYS, L2_VALUE = 15, 256, 4096
L1_SPAN, L0_SPAN = (1, 6), (1, 13)                 # the level-2 files each sparse table crosses


def l2_user(j: int, i: int) -> bytes:
    return b"key%03d%05d" % (j, 1000 + i)


def compaction_ops():
    """The script: level 2's flushes, the level-1 flush, the level-0 flush.
    Key (j, i) lies inside level-2 file j for i < L2_KEYS and in the gap behind
    it otherwise."""
    ops = []
    for j in range(L2_FILES):
        for i in range(L2_KEYS):
            ops.append(("p", l2_user(j, i), (b"%04d" % (j * 7 + i)) * (L2_VALUE // 4)))
        ops.append(("f",))
    for j in range(L1_SPAN[0], L1_SPAN[1] + 1):
        for i in range(0, 1000, 37):
            ops.append(("p", l2_user(j, i), b"%05d/%d/one" % (i, j)))
    ops.append(("f",))
    n = 0
    for j in range(L0_SPAN[0], L0_SPAN[1] + 1):
        for i in range(0, 1000, 23):
            n += 1
            if n % 5 == 0:
                ops.append(("d", l2_user(j, i)))
            elif n % 7 == 0 and j <= L1_SPAN[1]:
                ops.append(("d", l2_user(j, i // 37 * 37)))      # over a level-1 put
            else:
                ops.append(("p", l2_user(j, i), b"%05d/%d/zero" % (i, j)))
    ops.append(("f",))
    return ops


def levels_of(text: str):
    """[[(number, bytes, smallest, largest)] per level] of "leveldb.sstables"."""
    levels, level = [[] for _ in range(7)], None

    def key(m, at):
        return ikey(m.group(at).encode(), int(m.group(at + 1)), int(m.group(at + 2)))

    for ln in text.splitlines():
        m = re.match(r"--- level (\d+) ---", ln)
        if m:
            level = int(m.group(1))
            continue
        m = re.match(r" (\d+):(\d+)\['(\w+)' @ (\d+) : (\d+) \.\. '(\w+)' @ (\d+) : (\d+)\]$", ln)
        if m:
            levels[level].append((int(m.group(1)), int(m.group(2)), key(m, 3), key(m, 6)))
        else:
            assert not ln.strip(), ln
    return levels


def table_entries(img: bytes):
    st, es = scan(Table(img, internal=True, filter_name=None))
    assert st == ST_OK
    return es


def run_compaction(driver, tmp) -> Compaction:
    db, sp, od = (os.path.join(tmp, n) for n in ("db", "script", "out"))
    ops = compaction_ops()
    with open(sp, "wb") as f:
        f.write(struct.pack("<I", len(ops)))
        for op in ops:
            if op[0] == "p":
                f.write(struct.pack("<I", 0) + blob(op[1]) + blob(op[2]))
            elif op[0] == "d":
                f.write(struct.pack("<I", 1) + blob(op[1]))
            else:
                f.write(struct.pack("<I", 2))
    os.makedirs(od)
    subprocess.run([driver, "compact", db, sp, od], check=True, capture_output=True)
    before = levels_of(open(os.path.join(od, "stage0.txt")).read())
    after = levels_of(open(os.path.join(od, "stage1.txt")).read())
    assert [len(lv) for lv in before] == [1, 1, L2_FILES, 0, 0, 0, 0], [len(lv) for lv in before]
    assert before[2] == after[2] and not after[0] and len(after[1]) >= 2
    lv2 = [(lo, hi, size) for _, size, lo, hi in before[2]]
    assert sum(s for _, _, s in lv2) > 10 << 20 and all(900 << 10 < s < 1200 << 10 for _, _, s in lv2)
    last = sum(1 for op in ops if op[0] != "f")
    c = Compaction(4096, 16, 0, 0, 1 << 20, 1 << 20, last, levels=[lv2])
    inputs = []
    for num, size, lo, hi in before[0] + before[1]:     # the merging iterator's order
        img = open(os.path.join(od, "stage0", "%06d.ldb" % num), "rb").read()
        assert len(img) == size
        es = table_entries(img)
        assert (es[0][0], es[-1][0]) == (lo, hi)
        c.inputs.append(img)
        inputs.append(es)
    # Level-2 files wholly before and wholly behind the inputs.
    lo = min(es[0][0][:-8] for es in inputs)
    hi = max(es[-1][0][:-8] for es in inputs)
    assert lv2[0][1][:-8] < lo and lv2[-1][0][:-8] > hi
    merged = [inputs[r][i] for r, i in sim_merge.merge_serial(inputs, True)]
    outs = [open(os.path.join(od, "stage1", "%06d.ldb" % num), "rb").read()
            for num, _, _, _ in after[1]]
    kept, first, mine = sim.compact_serial(merged, last, [lv2], c.limit, 4096, 16, 0, 0, 1 << 20)
    assert mine == outs, "the model's files differ from lcdb's"
    assert sim.compact_parallel(merged, last, [lv2], c.limit, 4096, 16, 0, 0, 1 << 20) == \
        (kept, first, mine)
    for f, img in enumerate(outs):
        assert table_entries(img) == kept[first[f]:first[f + 1]]
        c.files.append(out_file(kept[first[f]:first[f + 1]], img, True))
    # What the compaction must show.
    stops, drops = sim.loop_serial([k for k, _ in merged], last, [lv2], c.limit)
    assert any(stops) and any(len(img) < (1 << 20) for img in outs[:-1]), \
        "no stop closed a file below max_output_file_size"
    ranges = [(a[:-8], b[:-8]) for a, b, _ in lv2]
    covered = lambda u: any(a <= u <= b for a, b in ranges)   # noqa: E731
    kept_dels = [k for k, _ in kept if k[-8] == 0]
    assert kept_dels and all(covered(k[:-8]) for k in kept_dels), "no deletion kept over a deeper file"
    first_dels = [k for i, (k, _) in enumerate(merged)
                  if k[-8] == 0 and drops[i] and (i == 0 or merged[i - 1][0][:-8] != k[:-8])]
    assert first_dels and not any(covered(k[:-8]) for k in first_dels), "no deletion dropped in a gap"
    # The loop mode, fed the same inputs and levels, writes the same files:
    # the driver's transcription of the loop is lcdb's loop.
    lc = LoopCase("compaction", 4096, 16, 0, 0, 1 << 20, 1 << 20, last, levels=[lv2], entries=merged)
    flags, counts, images = run_loop(driver, tmp, lc, "tie_")
    assert images == outs and counts == [f.entries for f in c.files]
    assert flags == bytes(STOP * s | DROP * d for s, d in zip(stops, drops))
    print(f"  compaction: {len(merged)} entries over {len(lv2)} level-2 files of "
          f"{sum(s for _, _, s in lv2)} bytes, {sum(stops)} stops -> {len(kept)} kept in "
          f"{len(outs)} files of {[len(i) for i in outs]} bytes; {len(kept_dels)} deletions kept, "
          f"{len(first_dels)} dropped in gaps")
    return c


def main() -> None:
    cases = loop_cases()
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        for c in cases:
            record_loop(driver, tmp, c)
        check_cases(cases)
        compact = run_compaction(driver, tmp)
    size = write(PATH, cases, compact)
    print(f"{PATH}: {len(cases)} loop cases, 1 compaction, {size} bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
