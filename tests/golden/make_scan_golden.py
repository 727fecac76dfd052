#!/usr/bin/env python3
"""Generate tests/golden/table_scan.bin from the REFERENCE table iterator.

Run where make_get_golden.py runs: beside the reference checkout, after
oracle/lcdb.mk has compiled it (oracle/_ref/lcdb/liblcdb_core.a, refsnappy.o);
never on the GPU box.  Compiles tests/golden/table_scan_driver.c against the reference's
headers, writes every case's table (a table of tests/golden/table_build.bin,
which lcdb's builder wrote, with the case's patches) to a temporary file and
records what lcdb's own ldb_tableiter_create + first / seek + next deliver:
a full scan, and seeks each followed by a scan to the end.  The digests are
hashlib's over the driver's output.  Nothing recorded was computed by the
code under test.

Usage: python tests/golden/make_scan_golden.py
       python tests/golden/make_scan_golden.py --time TABLE.ldb REPS
         (the reference's full scan loop on one core of this host)
"""
from __future__ import annotations

import hashlib
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import table_get_golden_io  # noqa: E402
import table_golden_io  # noqa: E402
from make_get_golden import CFLAGS, LCDB, MAX_SEQ, layout, le32, tag  # noqa: E402
from sim_table_get import decode_entry  # noqa: E402
from table_get_golden_io import patched  # noqa: E402
from table_io import block_entries, entry_offsets  # noqa: E402
from table_scan_golden_io import PATH, RECORD_MAX, Case, Run, write  # noqa: E402


def compile_driver(tmp: str) -> str:
    driver = os.path.join(tmp, "table_scan_driver")
    subprocess.run(["gcc", *CFLAGS, os.path.join(HERE, "table_scan_driver.c"),
                    os.path.join(LCDB, "refsnappy.o"), os.path.join(LCDB, "liblcdb_core.a"),
                    "-lpthread", "-o", driver], check=True)
    return driver


def run_driver(driver: str, tmp: str, table: bytes, c: Case, seeks, timeout=None) -> None:
    tp, cp, op = (os.path.join(tmp, n) for n in ("t.ldb", "case", "out"))
    with open(tp, "wb") as f:
        f.write(table)
    with open(cp, "wb") as f:
        f.write(struct.pack("<5I", c.internal, c.bits_per_key, c.paranoid, c.verify, len(seeks)))
        for k in seeks:
            f.write(struct.pack("<I", len(k)) + k)
    r = subprocess.run([driver, tp, cp, op], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    b = open(op, "rb").read()
    (c.open_rc,) = struct.unpack_from("<i", b, 0)
    at = 4
    if c.open_rc != 0:
        return
    for start in [None] + list(seeks):
        rc, count = struct.unpack_from("<iI", b, at)
        at += 8
        h, ents = hashlib.sha256(), []
        for _ in range(count):
            (kn,) = struct.unpack_from("<I", b, at)
            k = b[at + 4:at + 4 + kn]
            at += 4 + kn
            (vn,) = struct.unpack_from("<I", b, at)
            v = b[at + 4:at + 4 + vn]
            at += 4 + vn
            h.update(struct.pack("<I", kn) + k + struct.pack("<I", vn) + v)
            ents.append((k, v))
        c.runs.append(Run(start, rc, count, h.digest(), ents if count <= RECORD_MAX else None))
    assert at == len(b)


def seeks_of(entries, blocks, internal: int):
    """A stored key, a key between two blocks, a key past the end; and keys of
    block 0's first and third restart runs, where a damaged block's seek and
    its forward walk part ways."""
    stored = [k for k, _ in entries]
    if not stored:
        return [b"a" * 9, b"", b"\xff" * 9]

    def after(k):
        return (k[:-8] + b"\0" + tag(MAX_SEQ, 1)) if internal else k + b"\0"

    out = [stored[len(stored) // 2]]
    first_block = block_entries(blocks[0]) if blocks else []
    out.append(after(first_block[-1][0] if first_block else stored[0]))
    last = stored[-1]
    out.append((last[:-8] + b"\xff" + tag(MAX_SEQ, 1)) if internal else last + b"\xff")
    out += [stored[min(3, len(stored) - 1)], stored[min(40, len(stored) - 1)]]
    seen, uniq = set(), []
    for k in out:
        if k not in seen:
            seen.add(k)
            uniq.append(k)
    return uniq


def own_patches(sets):
    """[(name, set name, variant index, patches[, more seeks])]: where a forward
    walk and a seek differ.  Uncompressed tables read with verify_checksums = 0."""
    def find(set_name, want):
        s = next(x for x in sets if x.name == set_name)
        for i, v in enumerate(s.variants):
            if (v.block_size, v.restart_interval, v.compression, v.bits_per_key) == want:
                return s, i, v
        raise KeyError((set_name, want))

    out = []
    for sn in ("fill4096", "fill4096_internal"):
        s, vi, v = find(sn, (4096, 16, 0, 0))
        img = v.file
        ioff, idx, ents = layout(img)
        boff, bsize = ents[0][3]
        blk = img[boff:boff + bsize]
        eo = entry_offsets(blk)
        nr = struct.unpack_from("<I", blk, bsize - 4)[0]
        restarts = bsize - 4 * (nr + 1)
        rp = [struct.unpack_from("<I", blk, restarts + 4 * i)[0] for i in range(nr)]
        assert nr >= 3 and rp[1] == eo[16]
        # An entry of the second restart run whose `shared` exceeds the key
        # before it: the walk from restart[0] ends there, a seek into a later
        # run never sees it.
        out.append((f"{sn}:damage_before_later_restart", sn, vi, [(boff + eo[17], b"\x64")]))
        # Slot 0 of the restart array names the second run: first() begins there.
        out.append((f"{sn}:restart_slot0_not_0", sn, vi, [(boff + restarts, le32(rp[1]))]))
        # The same in the table's last block, so the scan ends in it.
        loff, lsize = ents[-1][3]
        lblk = img[loff:loff + lsize]
        lnr = struct.unpack_from("<I", lblk, lsize - 4)[0]
        leo = entry_offsets(lblk)
        if len(leo) >= 3:
            out.append((f"{sn}:damage_in_last_block", sn, vi, [(loff + leo[2], b"\x64")]))
        assert lnr >= 1
    # Index blocks whose entries do not line up with their restart slots.
    for sn in ("fill256", "fill4096_internal"):
        s, vi, v = find(sn, (256, 1, 0, 0) if sn == "fill256" else (4096, 16, 0, 0))
        ioff, idx, ents = layout(v.file)
        nr = struct.unpack_from("<I", idx, len(idx) - 4)[0]
        restarts = len(idx) - 4 * (nr + 1)
        assert nr == len(ents) and nr >= 4
        slot = [struct.unpack_from("<I", idx, restarts + 4 * i)[0] for i in range(nr)]
        mid = nr // 2
        # A slot that repeats its successor: every entry still parses in the
        # walk, but slot and entry numbers no longer agree.
        out.append((f"{sn}:index_slot_repeated", sn, vi,
                    [(ioff + restarts + 4 * mid, le32(slot[mid + 1]))]))
    # Two made-up entries inside index entry k's key bytes, the second ending
    # where entry k ends, and slot k pointing at the first: a seek for entry
    # k's old key parses on from slot k and finds the second made-up entry,
    # which the walk from restart[0] never visits; the two walks meet again at
    # entry k + 1.
    s, vi, v = find("fill256", (256, 1, 0, 0))
    ioff, idx, ents = layout(v.file)
    nr = struct.unpack_from("<I", idx, len(idx) - 4)[0]
    restarts = len(idx) - 4 * (nr + 1)
    for k in range(1, nr - 1):
        e = decode_entry(idx, ents[k][0], restarts)
        if e[0] == 0 and e[1] >= 12 and max(idx[ents[k][0]:ents[k][0] + 3]) < 128:
            at, n, vl = e[3], e[1], e[2]
            old = idx[at:at + n]
            na = (n - 6) // 2
            nb = n - 6 - na
            fake = bytes([0, na, 0]) + old[:na] + bytes([0, nb, vl]) + b"\xff" * nb
            assert len(fake) == n and old[0] != 0xff
            out.append(("fill256:index_seek_off_walk", "fill256", vi,
                        [(ioff + at, fake), (ioff + restarts + 4 * k, le32(at))], [old]))
            break
    else:
        raise AssertionError("no index entry to patch")
    return out


def time_reference(argv) -> None:
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        subprocess.run([driver, "--time", *argv], check=True)


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        return time_reference(sys.argv[2:])
    sets = table_golden_io.read()
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        for s in sets:
            internal = int(s.name.endswith("_internal"))
            for vi, v in enumerate(s.variants):
                c = Case(f"{s.name}:{vi}", s.name, vi, [], internal, v.bits_per_key, 0, 1)
                run_driver(driver, tmp, v.file, c, seeks_of(s.entries, v.blocks, internal))
                assert c.open_rc == 0 and c.runs[0].rc == 0
                assert c.runs[0].count == len(s.entries), c.name
                cases.append(c)
        for g in table_get_golden_io.read():
            if not g.patches:
                continue
            s = next(x for x in sets if x.name == g.set_name)
            v = s.variants[g.variant]
            c = Case(g.name, g.set_name, g.variant, g.patches, g.internal, g.bits_per_key,
                     g.paranoid, g.verify)
            run_driver(driver, tmp, table_get_golden_io.table_of(g, sets), c,
                       seeks_of(s.entries, v.blocks, g.internal))
            cases.append(c)
        for name, sn, vi, patches, *more in own_patches(sets):
            s = next(x for x in sets if x.name == sn)
            v = s.variants[vi]
            c = Case(name, sn, vi, patches, v.internal, v.bits_per_key, 0, 0)
            run_driver(driver, tmp, patched(v.file, patches), c,
                       seeks_of(s.entries, v.blocks, v.internal) + (more[0] if more else []))
            cases.append(c)
        for c in cases:
            if c.patches:
                print(f"  {c.name}: open={c.open_rc} " +
                      " ".join(f"{r.rc}/{r.count}" for r in c.runs))
    size = write(PATH, cases)
    print(f"{PATH}: {len(cases)} cases, {sum(len(c.runs) for c in cases)} runs, {size} bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
