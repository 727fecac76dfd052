#!/usr/bin/env python3
"""Generate tests/golden/table_build.bin from the REFERENCE table builder.

Run in the build container, where /root/reference exists and oracle/lcdb.mk
has compiled it (oracle/_ref/lcdb/liblcdb_core.a, refsnappy.o); never on the
GPU box.  Compiles tests/golden/table_golden_driver.c against the reference's
headers, feeds every case's entries to lcdb's own ldb_tablegen_* and records
the entries, the options and the file it wrote.  The raw data blocks and
index keys of a case are read out of a second, uncompressed build by the
reference (its index block's handles), so nothing recorded was computed by
the code under test.

Usage: python tests/golden/make_table_golden.py
"""
from __future__ import annotations

import os
import random
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from table_golden_io import PATH, EntrySet, Variant, write  # noqa: E402
from table_io import _varint, block_entries  # noqa: E402

REF = "/root/reference"
LCDB = os.path.join(ROOT, "oracle", "_ref", "lcdb")
CFLAGS = ["-std=c89", "-O2", "-D_GNU_SOURCE", "-DLDB_PTHREAD", "-DLDB_HAVE_FDATASYNC",
          "-DLDB_HAVE_PREAD", f"-I{REF}/include", f"-I{REF}/src"]      # oracle/lcdb.mk


def ik(user: bytes, seq: int, typ: int = 1) -> bytes:
    """An internal key (dbformat.c: user key | fixed64 seq << 8 | type)."""
    return user + struct.pack("<Q", (seq << 8) | typ)


def internal(entries):
    return [(ik(k, i + 1), v) for i, (k, v) in enumerate(entries)]


def run_driver(driver, tmp, entries, bs, R, comp, bpk, inter) -> bytes:
    case, out = os.path.join(tmp, "case"), os.path.join(tmp, "out.ldb")
    with open(case, "wb") as f:
        f.write(struct.pack("<6I", bs, R, comp, bpk, inter, len(entries)))
        for k, v in entries:
            f.write(struct.pack("<I", len(k)) + k + struct.pack("<I", len(v)) + v)
    r = subprocess.run([driver, case, out], capture_output=True, text=True)
    assert r.returncode == 0 and "rc=0" in r.stdout, r.stdout + r.stderr
    return open(out, "rb").read()


def raw_blocks(img: bytes):
    """(data blocks, index keys) of an uncompressed table, through its footer
    and index block (format.c:92-137)."""
    foot = img[-48:]
    _, at = _varint(foot, 0, 40, 64)
    _, at = _varint(foot, at, 40, 64)
    ioff, at = _varint(foot, at, 40, 64)
    isize, at = _varint(foot, at, 40, 64)
    assert img[ioff + isize] == 0
    blocks, keys = [], []
    for k, h in block_entries(img[ioff:ioff + isize]):
        off, p = _varint(h, 0, len(h), 64)
        size, _ = _varint(h, p, len(h), 64)
        assert img[off + size] == 0
        blocks.append(img[off:off + size])
        keys.append(k)
    return blocks, keys


def patterned(rng: random.Random, n: int) -> bytes:
    """Compressible bytes: short random words repeated."""
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(6, 17))) for _ in range(12)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words)
    return bytes(out[:n])


def cases():
    """[(name, bytewise entries or None, internal entries or None, variants)],
    a variant = (block_size, restart_interval, compression, bits_per_key)."""
    rng = random.Random(4242)
    out = []
    for n in (0, 1, 15, 16, 17, 33, 49):          # entries per block: the restart boundaries
        e = [(b"key%06d" % (3 * i), patterned(rng, 10)) for i in range(n)]
        v = [(4096, 16, 1, 0)]
        if n in (0, 17):
            v.append((4096, 16, 0, 10))
        out.append((f"count{n}", e, internal(e), v))
    e = [(b"%016d" % i, patterned(rng, 20)) for i in range(40)]
    out.append(("own_block", e, internal(e), [(1, 16, 1, 10), (1, 16, 0, 0)]))
    e = [(b"%016d" % i, patterned(rng, 100)) for i in range(60)]
    out.append(("fill256", e, internal(e), [(256, 16, 1, 0), (256, 16, 0, 10), (256, 2, 1, 10),
                                            (256, 1, 0, 0)]))
    e = [(b"%016d" % i, patterned(rng, 100)) for i in range(150)]
    out.append(("fill4096", e, internal(e), [(4096, 16, 1, 10), (4096, 16, 0, 0)]))
    # Varint edges: shared, non_shared and value length on each side of
    # 127/128 and 16383/16384.
    ks = [b"a" * 127 + b"b", b"a" * 127 + b"c", b"a" * 128 + b"b", b"a" * 128 + b"c",
          b"a" * 128 + b"d" + b"x" * 126, b"a" * 128 + b"e" + b"x" * 127,
          b"b" * 16383 + b"c", b"b" * 16383 + b"d", b"b" * 16384 + b"c", b"b" * 16384 + b"d",
          b"c" + b"y" * 16382, b"d" + b"y" * 16383, b"e" * 126, b"e" * 127, b"f" * 128]
    vls = [0, 127, 128, 16383, 16384]
    e = [(k, patterned(rng, vls[i % 5])) for i, k in enumerate(sorted(ks))]
    out.append(("varint", e, internal(e), [(1 << 20, 64, 1, 0), (65536, 16, 0, 10)]))
    e = [(b"", b"v0"), (b"a", b""), (b"ab", b"x"), (b"abc", b""), (b"b", b"nothing shared"),
         (b"zzz", b"q")]
    out.append(("shapes", e, None, [(4096, 16, 1, 0), (1, 16, 0, 10), (30, 2, 1, 10)]))
    e = [(b"big%02d" % i, patterned(rng, 70000 if i == 2 else 50)) for i in range(5)]
    out.append(("bigvalue", e, internal(e), [(4096, 16, 1, 0)]))
    # Separators: block_size 1 makes every neighbouring pair a block boundary.
    us = [b"k\xfe1", b"k\xff1",                    # differing byte + 1 is 0xff: kept
          b"m\x10zz", b"m\xffzz",                  # limit's byte 0xff: shortened
          b"p1aa", b"p2aa",                        # differing byte + 1 = limit's byte: kept
          b"q", b"qa",                             # a prefix of the next: kept
          b"r1xxxx", b"r5",                        # shortened
          b"s1", b"s5zz",                          # shortened in place (same length)
          b"t\xff\xff", b"u"]
    e = [(k, b"v%d" % i) for i, k in enumerate(us)]
    ie = internal(e)
    # Equal user keys with decreasing sequence numbers across a boundary.
    ie += [(ik(b"v", 9), b"new"), (ik(b"v", 5), b"old"), (ik(b"w1xxxx", 3), b""), (ik(b"w7", 2), b"")]
    out.append(("separators", e, ie, [(1, 16, 1, 0), (1, 16, 0, 10)]))
    for nm, last in (("succ_ff", b"\xff\xff\xff"), ("succ_inc", b"abc"), ("succ_mid", b"\xff\xffa"),
                     ("succ_one", b"\xff\xfe")):
        e = [(b"\x01", b"first"), (last, b"last")]
        out.append((nm, e, internal(e), [(4096, 16, 1, 0)]))
    return out


def main() -> None:
    sets = []
    with tempfile.TemporaryDirectory() as tmp:
        driver = os.path.join(tmp, "table_golden_driver")
        subprocess.run(["gcc", *CFLAGS, os.path.join(HERE, "table_golden_driver.c"),
                        os.path.join(LCDB, "refsnappy.o"), os.path.join(LCDB, "liblcdb_core.a"),
                        "-lpthread", "-o", driver], check=True)
        for name, plain, inter, variants in cases():
            for kind, entries in ((0, plain), (1, inter)):
                if entries is None:
                    continue
                vs = []
                for bs, R, comp, bpk in variants:
                    v = Variant(bs, R, comp, bpk, kind)
                    v.file = run_driver(driver, tmp, entries, bs, R, comp, bpk, kind)
                    v.blocks, v.ikeys = raw_blocks(run_driver(driver, tmp, entries, bs, R, 0, 0, kind))
                    got = [x for b in v.blocks for x in block_entries(b)]
                    assert got == entries, name
                    vs.append(v)
                sets.append(EntrySet(name + ("_internal" if kind else ""), entries, vs))
    size = write(PATH, sets)
    nv = sum(len(s.variants) for s in sets)
    print(f"{PATH}: {len(sets)} entry sets, {nv} tables, {size} bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
