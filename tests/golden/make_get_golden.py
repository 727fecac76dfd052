#!/usr/bin/env python3
"""Generate tests/golden/table_get.bin from the REFERENCE table reader.

Run in the build container, where /root/reference exists and oracle/lcdb.mk
has compiled it (oracle/_ref/lcdb/liblcdb_core.a, refsnappy.o); never on the
GPU box.  Compiles tests/golden/table_get_driver.c against the reference's
headers, writes every case's table (a table of tests/golden/table_build.bin,
which lcdb's builder wrote, with the case's patches) to a temporary file and
records what lcdb's own ldb_table_open + ldb_table_internal_get return for
the case's queries.  Nothing recorded was computed by the code under test.

Usage: python tests/golden/make_get_golden.py
       python tests/golden/make_get_golden.py --time TABLE.ldb KEYS REPS
         (the reference's lookup loop on one core of this host; KEYS: a case
          file as the driver reads it)
"""
from __future__ import annotations

import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import table_golden_io  # noqa: E402
from table_get_golden_io import PATH, Case, Record, patched, write  # noqa: E402
from table_io import _varint, entry_offsets  # noqa: E402

REF = "/root/reference"
LCDB = os.path.join(ROOT, "oracle", "_ref", "lcdb")
CFLAGS = ["-std=c89", "-O2", "-D_GNU_SOURCE", "-DLDB_PTHREAD", "-DLDB_HAVE_FDATASYNC",
          "-DLDB_HAVE_PREAD", f"-I{REF}/include", f"-I{REF}/src"]      # oracle/lcdb.mk

MAX_SEQ = (1 << 56) - 1


def tag(seq: int, typ: int) -> bytes:
    return struct.pack("<Q", (seq << 8) | typ)


def compile_driver(tmp: str) -> str:
    driver = os.path.join(tmp, "table_get_driver")
    subprocess.run(["gcc", *CFLAGS, os.path.join(HERE, "table_get_driver.c"),
                    os.path.join(LCDB, "refsnappy.o"), os.path.join(LCDB, "liblcdb_core.a"),
                    "-lpthread", "-o", driver], check=True)
    return driver


def case_file(path: str, internal: int, bits: int, paranoid: int, verify: int, keys) -> None:
    with open(path, "wb") as f:
        f.write(struct.pack("<5I", internal, bits, paranoid, verify, len(keys)))
        for k in keys:
            f.write(struct.pack("<I", len(k)) + k)


def run_driver(driver: str, tmp: str, table: bytes, c: Case, keys, timeout=None) -> None:
    tp, cp, op = (os.path.join(tmp, n) for n in ("t.ldb", "case", "out"))
    with open(tp, "wb") as f:
        f.write(table)
    case_file(cp, c.internal, c.bits_per_key, c.paranoid, c.verify, keys)
    r = subprocess.run([driver, tp, cp, op], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    b = open(op, "rb").read()
    (c.open_rc,) = struct.unpack_from("<i", b, 0)
    at = 4
    if c.open_rc != 0:
        return
    for k in keys:
        rc, called, kn = struct.unpack_from("<iBI", b, at)
        at += 9
        fk = b[at:at + kn]
        at += kn
        (vn,) = struct.unpack_from("<I", b, at)
        at += 4
        c.records.append(Record(k, rc, called, fk, b[at:at + vn]))
        at += vn
    assert at == len(b)


def bump(k: bytes, d: int) -> bytes:
    return k[:-1] + bytes([(k[-1] + d) & 255]) if k else k


def queries(entries, ikeys, internal: int, budget: int = 320):
    """The lookups of one table: every stored key, and around the stored keys
    (all of them while the table stays within `budget` lookups, else evenly
    spaced ones) the neighbours a seek can confuse them with."""
    stored = [k for k, _ in entries]
    out = list(stored)
    per = 10 if internal else 4
    step = max(1, -(-len(stored) * per // max(1, budget - len(stored))))
    for k in stored[::step]:
        out += [bump(k, 1), bump(k, -1), k[:-1], k + b"\0"]
        if internal:
            u, t = k[:-8], struct.unpack("<Q", k[-8:])[0]
            out += [u + tag(MAX_SEQ, 1), u + tag(0, 1), u + tag(0, 0),
                    u + struct.pack("<Q", (t + 1) & (2**64 - 1)),
                    u + struct.pack("<Q", (t - 1) & (2**64 - 1)),
                    bump(u, 1) + tag(MAX_SEQ, 1), bump(u, -1) + tag(MAX_SEQ, 1),
                    u[:-1] + tag(MAX_SEQ, 1), u + b"\0" + tag(MAX_SEQ, 1)]
    out += list(ikeys)
    out.append(b"")
    last = stored[-1] if stored else b"x" * 9
    out.append((last[:-8] + b"\xff" + tag(MAX_SEQ, 1)) if internal else last + b"\xff")
    if internal:
        out += [b"abcdefg"[:n] for n in range(8)]       # targets under 8 bytes
    seen, uniq = set(), []
    for k in out:
        if k not in seen:
            seen.add(k)
            uniq.append(k)
    return uniq


def layout(img: bytes):
    """Of an uncompressed table: (index offset, index contents, [(entry offset
    in the index block, value offset, value length, (block offset, size))])."""
    foot = img[-48:]
    _, at = _varint(foot, 0, 40, 64)
    _, at = _varint(foot, at, 40, 64)
    ioff, at = _varint(foot, at, 40, 64)
    isize, at = _varint(foot, at, 40, 64)
    assert img[ioff + isize] == 0
    idx = img[ioff:ioff + isize]
    nr = struct.unpack_from("<I", idx, isize - 4)[0]
    limit = isize - 4 * (nr + 1)
    ents = []
    for e in entry_offsets(idx):
        sh, p = _varint(idx, e, limit, 32)
        ns, p = _varint(idx, p, limit, 32)
        vl, p = _varint(idx, p, limit, 32)
        v = p + ns
        off, q = _varint(idx, v, v + vl, 64)
        size, _ = _varint(idx, q, v + vl, 64)
        assert sh == 0 and img[off + size] == 0
        ents.append((e, v, vl, (off, size)))
    return ioff, idx, ents


def le32(x: int) -> bytes:
    return struct.pack("<I", x)


def patch_cases(sets):
    """[(name, set name, variant index, patches, verify)] on uncompressed
    tables read with verify_checksums = 0, so the bytes reach the iterator."""
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
        assert nr >= 3 and len(ents) >= 2
        restarts = bsize - 4 * (nr + 1)
        rp = [struct.unpack_from("<I", blk, restarts + 4 * i)[0] for i in range(nr)]
        mid = (0 + nr - 1 + 1) // 2
        last = eo[-1]
        assert max(blk[last:last + 3]) < 128 and blk[last + 2] >= 3
        add = lambda name, patches: out.append((f"{sn}:{name}", sn, vi, patches, 0))  # noqa: E731
        add("restart_count_0", [(boff + bsize - 4, le32(0))])
        add("restart_count_over", [(boff + bsize - 4, le32((bsize - 4) // 4 + 1))])
        # The handle's size re-encoded in as many bytes as it had (a padded
        # varint), and a raw type byte behind the three bytes it leaves.
        e, vo, vl, (ho, hs) = ents[0]
        _, p = _varint(idx, vo, vo + vl, 64)
        width = vo + vl - p
        assert width >= 2
        three = bytes([0x83] + [0x80] * (width - 2) + [0x00])
        add("block_of_3_bytes", [(ioff + p, three), (ho + 3, b"\0")])
        add("restart_offset_past_array", [(boff + restarts + 4 * mid, le32(0xffffff00))])
        add("restart_shared_nonzero", [(boff + rp[mid], b"\x01")])
        add("shared_over_previous_key", [(boff + eo[1], b"\x64")])
        # (The last key is made smaller, so that the lookup of the key it was
        # scans past it: the index sends nothing larger to this block.)
        kend = last + 3 + blk[last + 1] - (9 if sn.endswith("_internal") else 1)
        add("varint_into_restart_array",
            [(boff + last + 2, bytes([blk[last + 2] - 3])), (boff + restarts - 3, b"\x81\x81\x81"),
             (boff + kend, bytes([blk[kend] - 1]))])
        add("lengths_over_limit", [(boff + last + 2, b"\x7f")])
        add("index_value_no_handle", [(ioff + vo, b"\xff" * vl)])
        e1, vo1, vl1, _ = ents[1]
        assert vl1 >= 4 and 2 * 16383 > len(img)
        add("handle_past_file_end", [(ioff + vo1, (b"\xff\x7f" * vl1)[:vl1 - 1] + b"\x7f")])
        # Unsorted: a later entry's key delta made smaller than its
        # predecessors', and a restart key made larger than its successors'.
        d5 = eo[5] + 3
        add("unsorted_scan", [(boff + d5, b"\x00")])
        add("unsorted_restart", [(boff + rp[1] + 3, b"\x7e")])
        if sn.endswith("_internal"):
            add("internal_key_under_8", [(boff + eo[2], b"\x00\x03")])
            add("internal_restart_key_under_8", [(boff + rp[mid] + 1, b"\x07")])
    s, vi, v = find("fill256", (256, 1, 0, 0))
    _, _, ents = layout(v.file)
    boff, bsize = ents[0][3]
    eo = entry_offsets(v.file[boff:boff + bsize])
    k0 = v.file[boff + eo[0] + 3:boff + eo[0] + 19]
    k1 = v.file[boff + eo[1] + 3:boff + eo[1] + 19]
    out.append(("fill256:unsorted_restart_keys", "fill256", vi,
                [(boff + eo[0] + 3, k1), (boff + eo[1] + 3, k0)], 0))
    # A compressed table with one flipped payload byte, checked and unchecked.
    s, vi, v = find("fill256", (256, 16, 1, 0))
    flip = [(40, bytes([v.file[40] ^ 0x55]))]
    out.append(("fill256:flipped_payload_verified", "fill256", vi, flip, 1))
    out.append(("fill256:flipped_payload_unverified", "fill256", vi, flip, 0))
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
                assert v.internal == internal
                c = Case(f"{s.name}:{vi}", s.name, vi, [], internal, v.bits_per_key, 0, 1)
                run_driver(driver, tmp, v.file, c, queries(s.entries, v.ikeys, internal))
                assert c.open_rc == 0
                hits = sum(r.called for r in c.records)
                assert hits >= len(s.entries), (c.name, hits)
                cases.append(c)
        for name, sn, vi, patches, verify in patch_cases(sets):
            s = next(x for x in sets if x.name == sn)
            v = s.variants[vi]
            c = Case(name, sn, vi, patches, v.internal, v.bits_per_key, 0, verify)
            run_driver(driver, tmp, patched(v.file, patches), c,
                       queries(s.entries, v.ikeys, v.internal, budget=200))
            bad = sum(r.rc != 0 for r in c.records)
            print(f"  {name}: open={c.open_rc} failing lookups {bad}/{len(c.records)}")
            cases.append(c)
    size = write(PATH, cases)
    nq = sum(len(c.records) for c in cases)
    print(f"{PATH}: {len(cases)} cases, {nq} lookups, {size} bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
