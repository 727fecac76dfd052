#!/usr/bin/env python3
"""Generate tests/golden/merge.bin from the REFERENCE merging iterator and the
REFERENCE's own compactions.

Run where make_scan_golden.py runs: beside the reference checkout, after
oracle/lcdb.mk has compiled it (oracle/_ref/lcdb/liblcdb_core.a, refsnappy.o);
never on the GPU box.  Compiles tests/golden/merge_driver.c against the
reference's headers.

Merge cases: every run becomes a table (one of tests/golden/table_build.bin,
which lcdb's builder wrote, or a new one through the driver's `build` mode,
lcdb's builder again), and the driver records what ldb_mergeiter_create over
one ldb_tableiter_create per table delivers, first + next until invalid.

Compaction steps: the driver opens a fresh DB (default options, no
compression), applies a script of puts, deletes, snapshots and memtable
flushes so that the files land in levels 2, 1, 0, 0, and runs
ldb_test_compact_range at level 0 (not base level: drop_deletions = 0) and at
level 1 (base level: drop_deletions = 1).  The input and output tables of both
steps are copied out and parsed here with tools/sim_table_scan.py.

Nothing recorded was computed by the code under test; tools/sim_merge.py must
reproduce every recorded output before the fixture is written.

Usage: python tests/golden/make_merge_golden.py
       python tests/golden/make_merge_golden.py --time INTERNAL REPS T1.ldb [T2.ldb ...]
         (the reference's merging loop on one core of this host)
       python tests/golden/make_merge_golden.py --time-deal K N REPS
         (the same over tools/bench_merge.py's workload: N fillseq entries
          dealt into K tables; recorded in profiles/merge_reference.json)
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

import sim_merge  # noqa: E402
import table_golden_io  # noqa: E402
from make_get_golden import CFLAGS, LCDB, tag  # noqa: E402
from merge_golden_io import (PATH, RECORD_MAX, CompactStep, MergeCase, Run, digest,  # noqa: E402
                             write)
from sim_table_scan import ST_OK, Table, scan  # noqa: E402


def compile_driver(tmp: str) -> str:
    driver = os.path.join(tmp, "merge_driver")
    subprocess.run(["gcc", *CFLAGS, os.path.join(HERE, "merge_driver.c"),
                    os.path.join(LCDB, "refsnappy.o"), os.path.join(LCDB, "liblcdb_core.a"),
                    "-lpthread", "-o", driver], check=True)
    return driver


def blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


def build_table(driver: str, tmp: str, name: str, entries, internal: int) -> str:
    cp, tp = os.path.join(tmp, "case"), os.path.join(tmp, name)
    with open(cp, "wb") as f:
        f.write(struct.pack("<6I", 4096, 16, 0, 0, internal, len(entries)))
        for k, v in entries:
            f.write(blob(k) + blob(v))
    subprocess.run([driver, "build", cp, tp], check=True)
    return tp


def parse_entries(b: bytes):
    rc, count = struct.unpack_from("<iI", b, 0)
    at, out = 8, []
    for _ in range(count):
        (kn,) = struct.unpack_from("<I", b, at)
        k = b[at + 4:at + 4 + kn]
        at += 4 + kn
        (vn,) = struct.unpack_from("<I", b, at)
        out.append((k, b[at + 4:at + 4 + vn]))
        at += 4 + vn
    assert at == len(b)
    return rc, out


# ---- merge cases -----------------------------------------------------------

def ik(user: bytes, seq: int, typ: int = 1) -> bytes:
    return user + tag(seq, typ)


def isorted(es):
    return sorted(es, key=sim_merge.sort_key(True))


def merge_cases(sets):
    def whole(name):
        s = next(x for x in sets if x.name == name)
        return Run(name, 0, len(s.entries), 1)

    def deal(name, k):
        s = next(x for x in sets if x.name == name)
        return [Run(name, r, len(s.entries), k) for r in range(k)]

    out = []
    for sfx, internal in (("", 0), ("_internal", 1)):
        f4, f2 = "fill4096" + sfx, "fill256" + sfx
        out.append(MergeCase("alone" + sfx, internal, [whole(f4)]))
        out.append(MergeCase("self" + sfx, internal, [whole(f4), whole(f4)]))
        out.append(MergeCase("deal3" + sfx, internal, deal(f4, 3)))
        out.append(MergeCase("deal7" + sfx, internal, deal(f4, 7)))
        e = deal(f2, 2)
        out.append(MergeCase("empty_among" + sfx, internal,
                             [e[0], whole("count0" + sfx), e[1], whole("count0" + sfx)]))
        out.append(MergeCase("no_tables" + sfx, internal, []))
        # One entry against thousands: between two keys, and on a key (a tie
        # the other run's value tells apart), from either side.
        big = [(b"key%08d" % (3 * i), b"%04d" % (i % 7919)) for i in range(3000)]
        between, on = (b"key%08d" % 4501, b"one"), (b"key%08d" % 4500, b"one")
        if internal:
            big = [(ik(k, 9), v) for k, v in big]
            between, on = (ik(between[0], 9), b"one"), (ik(on[0], 9), b"one")
        out.append(MergeCase("one_vs_thousands" + sfx, internal, [Run(own=[between]), Run(own=big)]))
        out.append(MergeCase("thousands_vs_one_tie" + sfx, internal, [Run(own=big), Run(own=[on])]))
        out.append(MergeCase("one_tie_vs_thousands" + sfx, internal, [Run(own=[on]), Run(own=big)]))
        # Values of 0 bytes and of several KiB.
        vals = [(b"v%03d" % i, bytes([65 + i % 26]) * (0 if i % 3 == 0 else 5000 + i))
                for i in range(12)]
        if internal:
            vals = [(ik(k, 3), v) for k, v in vals]
        out.append(MergeCase("value_sizes" + sfx, internal,
                             [Run(own=vals[0::2]), Run(own=vals[1::2])]))
    # Bytewise keys that agree in their first 8, 9 and 16 bytes, that are
    # prefixes of each other, and that are 300 bytes long.
    p8, p9, p16 = b"ABCDEFGH", b"ABCDEFGHI", b"ABCDEFGHIJKLMNOP"
    long_ = b"L" * 299
    keys = [b"", b"\0", b"ab", b"ab\0", b"ab\0\0", b"abc", p8, p8 + b"\0", p8 + b"a", p8 + b"b",
            p9, p9 + b"x", p9 + b"y", p16, p16 + b"0", p16 + b"1", p16 + b"1\0",
            long_ + b"a", long_ + b"b", long_, b"ABCDEFG", b"ABCDEFG\0"]
    keys = sorted(keys)
    es = [(k, b"%d" % i) for i, k in enumerate(keys)]
    out.append(MergeCase("prefixes", 0, [Run(own=es[r::3]) for r in range(3)]))
    # The same keys in every run, the value naming the run: the tie order.
    out.append(MergeCase("ties_by_run", 0,
                         [Run(own=[(k, b"run%d" % r) for k in keys]) for r in range(5)]))
    # Internal keys: a user key that is a prefix of another (the raw bytes of
    # the whole internal key order these wrongly), and one user key in several
    # runs with different sequences.
    users = [b"", b"ab", b"ab\0", b"ab\x01", b"ab\x01\x05", b"abc", p8, p8 + b"\0", p8 + b"\xff",
             p16, p16 + b"\x01"]
    runs = []
    for r in range(4):
        es = []
        for j, u in enumerate(users):
            if (j + r) % 4 != 3:
                es.append((ik(u, 10 * (j + 1) + r, (j + r) % 2), b"r%du%d" % (r, j)))
            if j % 3 == 0:
                es.append((ik(u, 200 + 7 * r + j), b"R%du%d" % (r, j)))
        runs.append(Run(own=isorted(es)))
    out.append(MergeCase("user_key_prefixes_internal", 1, runs))
    return out


def run_merge_case(driver, tmp, c: MergeCase, sets) -> None:
    paths = []
    for i, r in enumerate(c.runs):
        es = r.entries(sets)
        if r.set_name and (r.start, r.step) == (0, 1):
            s = next(x for x in sets if x.name == r.set_name)
            v = next(v for v in s.variants if v.compression == 0) if any(
                v.compression == 0 for v in s.variants) else s.variants[0]
            tp = os.path.join(tmp, f"t{i}.ldb")
            with open(tp, "wb") as f:
                f.write(v.file)
        else:
            tp = build_table(driver, tmp, f"t{i}.ldb", es, c.internal)
        paths.append(tp)
    op = os.path.join(tmp, "out")
    subprocess.run([driver, "merge", str(c.internal), op, *paths], check=True,
                   capture_output=True)
    c.status, got = parse_entries(open(op, "rb").read())
    c.count, c.digest = len(got), digest(got)
    c.entries = got if len(got) <= RECORD_MAX else None
    runs = [r.entries(sets) for r in c.runs]
    assert c.status == 0 and c.count == sum(len(r) for r in runs), c.name
    mine, src, dropped = sim_merge.merge(runs, bool(c.internal))
    assert mine == got and dropped == 0, c.name
    assert src == sim_merge.merge_serial(runs, bool(c.internal)), c.name


# ---- compaction steps ------------------------------------------------------

def scenarios():
    """[(name, [operation])]: four flushed groups over one key range each, so
    that the files land in levels 2, 1, 0, 0 (pick_level_for_memtable_output),
    with a snapshot nowhere, before every write, or after group 1, 2 or 3."""
    def edge(g):
        return [("p", b"a-lo", b"lo%d" % g), ("p", b"z-hi", b"hi%d" % g)]

    fill = [("p", b"fill%03d" % i, b"f" * (i % 50)) for i in range(60)]
    groups = [
        edge(1) + fill + [("p", b"k1", b"v1a"), ("p", b"k2", b"v2a"), ("p", b"d1", b"x1"),
                          ("p", b"d3", b"x3"), ("d", b"gone")],
        edge(2) + [("p", b"k1", b"v1b"), ("p", b"d2", b"y2"), ("d", b"d3"), ("p", b"k4", b"")],
        edge(3) + [("p", b"k1", b"v1c"), ("d", b"d1"), ("p", b"d3", b"x3again"),
                   ("p", b"k4", b"v4c"), ("d", b"k4")],
        edge(4) + [("p", b"k3", b"v3d"), ("d", b"d2"), ("p", b"k1", b"v1d"), ("d", b"never")],
    ]
    out = []
    for name, where in (("no_snapshot", None), ("snapshot_before_all", 0),
                        ("snapshot_after_group1", 1), ("snapshot_after_group2", 2),
                        ("snapshot_after_group3", 3)):
        ops = [("s",)] if where == 0 else []
        for g, grp in enumerate(groups, 1):
            ops += grp + [("f",)]
            if where == g:
                ops.append(("s",))
        out.append((name, ops))
    return out


def write_script(path: str, ops) -> tuple:
    """Returns (smallest_snapshot, last sequence): a write takes the next
    sequence, a snapshot holds the last one written."""
    seq, snap = 0, None
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(ops)))
        for op in ops:
            if op[0] == "p":
                seq += 1
                f.write(struct.pack("<I", 0) + blob(op[1]) + blob(op[2]))
            elif op[0] == "d":
                seq += 1
                f.write(struct.pack("<I", 1) + blob(op[1]))
            elif op[0] == "f":
                f.write(struct.pack("<I", 2))
            else:
                snap = seq if snap is None else snap
                f.write(struct.pack("<I", 3))
    return (seq if snap is None else snap), seq


def stage(outdir: str, k: int):
    """([[file number] per level], {number: image}, [files-at-level property])."""
    levels, level, props = [[] for _ in range(7)], None, []
    for ln in open(os.path.join(outdir, f"stage{k}.txt")).read().splitlines():
        m = re.match(r"--- level (\d+) ---", ln)
        if m:
            level = int(m.group(1))
            continue
        m = re.match(r" (\d+):(\d+)\[", ln)
        if m:
            levels[level].append(int(m.group(1)))
            continue
        m = re.match(r"files-at-level (\d+) (\d+)$", ln)
        if m:
            props.append(int(m.group(2)))
    files = {}
    for lv in levels:
        for num in lv:
            files[num] = open(os.path.join(outdir, f"stage{k}", "%06d.ldb" % num), "rb").read()
    assert props == [len(lv) for lv in levels[:4]], (props, levels)
    return levels, files


def table_entries(img: bytes):
    st, es = scan(Table(img, internal=True, filter_name=None))
    assert st == ST_OK
    return es


def run_scenario(driver, tmp, name, ops):
    db, sp, od = (os.path.join(tmp, n) for n in ("db_" + name, "script_" + name, "out_" + name))
    smallest, last = write_script(sp, ops)
    os.makedirs(od)
    subprocess.run([driver, "compact", db, sp, od], check=True, capture_output=True)
    s0, s1, s2 = stage(od, 0), stage(od, 1), stage(od, 2)
    assert [len(lv) for lv in s0[0][:4]] == [2, 1, 1, 0], (name, s0[0])
    assert [len(lv) for lv in s1[0][:4]] == [0, 1, 1, 0], (name, s1[0])
    assert [len(lv) for lv in s2[0][:4]] == [0, 0, 1, 0], (name, s2[0])
    seqs = [sim_merge.tag_of(k) >> 8 for img in s0[1].values() for k, _ in table_entries(img)]
    assert max(seqs) == last and len(seqs) == last and smallest <= last, name
    steps = []
    for which, before, after, level, dd in ((0, s0, s1, 0, 0), (1, s1, s2, 1, 1)):
        nums = before[0][level] + before[0][level + 1]
        (out_num,) = after[0][level + 1]
        assert out_num not in before[1], name
        img = after[1][out_num]
        st = CompactStep(f"{name}:level{level}", smallest, dd, 4096, 16, 0, 0,
                         [(before[1][n], table_entries(before[1][n])) for n in nums],
                         hashlib.sha256(img).digest(), len(img), table_entries(img))
        got, _, dropped = sim_merge.merge([es for _, es in st.inputs], True, True, smallest, bool(dd))
        assert got == st.out_entries, st.name
        keys = [k for k, _ in sim_merge.merge([es for _, es in st.inputs], True)[0]]
        assert sim_merge.drop_flags(keys, smallest, bool(dd)) == \
            sim_merge.drop_serial(keys, smallest, bool(dd)), st.name
        print(f"  {st.name}: snapshot {smallest}/{last}, {len(st.inputs)} files, "
              f"{sum(len(e) for _, e in st.inputs)} -> {len(st.out_entries)} entries ({dropped} dropped)")
        steps.append(st)
    return steps


def time_reference(argv) -> None:
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        subprocess.run([driver, "--time", *argv], check=True)


def time_deal(k: int, n: int, reps: int) -> None:
    """tools/bench_merge.py's workload through the reference: n fillseq entries
    dealt round-robin into k tables (lcdb's builder, no compression), merged by
    the driver's --time loop.  Adds "k<k>" to profiles/merge_reference.json."""
    import json

    from bench_merge import deal_runs
    from bench_table_build import fillseq_entries
    e = fillseq_entries(n)
    path = os.path.join(ROOT, "profiles", "merge_reference.json")
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        paths = []
        for r, run in enumerate(deal_runs(e, n, k)):
            kk, vv, m = run[0][:24 * run[6]].reshape(-1, 24), run[3][:100 * run[6]].reshape(-1, 100), run[6]
            es = [(kk[i].tobytes(), vv[i].tobytes()) for i in range(m)]
            paths.append(build_table(driver, tmp, f"t{r}.ldb", es, 1))
        r = subprocess.run([driver, "--time", "1", str(reps), *paths], check=True,
                           capture_output=True, text=True)
    print(r.stdout.strip())
    f = dict(x.split("=") for x in r.stdout.split())
    assert int(f["entries"]) == n and int(f["tables"]) == k
    ref = json.load(open(path)) if os.path.exists(path) else {
        "what": "lcdb's own ldb_mergeiter_create over one ldb_tableiter_create per table, "
                "ldb_iter_first + ldb_iter_next until invalid (tests/golden/merge_driver.c "
                "--time), internal-key comparator, one core, no block cache, files in the page "
                "cache, verify_checksums = 1, uncompressed 4 KiB blocks, best pass; the loop "
                "includes reading and walking the tables' blocks",
        "host": "the build host, NOT the MI355X host"}
    ref[f"k{k}"] = {"runs": k, "entries": n, "reps": reps,
                    "ns_per_entry": float(f["ns_per_entry"]), "ns_per_merge": float(f["ns_per_merge"])}
    with open(path, "w") as out:
        json.dump(ref, out, indent=1, sort_keys=True)
        out.write("\n")


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        return time_reference(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--time-deal":
        return time_deal(*(int(x) for x in sys.argv[2:5]))
    sets = table_golden_io.read()
    merges, steps = merge_cases(sets), []
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        for c in merges:
            run_merge_case(driver, tmp, c, sets)
        for name, ops in scenarios():
            steps += run_scenario(driver, tmp, name, ops)
    size = write(PATH, merges, steps)
    print(f"{PATH}: {len(merges)} merges, {len(steps)} compaction steps, {size} bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
