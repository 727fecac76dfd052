"""Reader/writer for tests/golden/table_scan.bin: what lcdb's own table
iterator (ldb_tableiter_create, first or seek, next until invalid) delivered
for the tables of tests/golden/table_build.bin, plain and patched
(tests/golden/make_scan_golden.py).

A case names its table by entry set and variant index of table_build.bin and
does not repeat its bytes; a patched table is the list of (offset, new bytes)
applied to it.  The file is one zlib stream of (little-endian):
    magic  b"LGSTSCN1"
    u32    cases
    per case:
        u16 name length, name (utf-8)             -- what the case is about
        u16 set name length, set name; u32 variant index
        u32 patches; per patch: u32 offset, u32 length, bytes
        u8 internal_keys, u8 bits_per_key, u8 paranoid_checks, u8 verify_checksums
        i32 rc of ldb_table_open
        u32 runs; per run: u8 has_start; u32 length, start key
                           i32 final rc of the iterator, u32 entries
                           32 bytes: SHA-256 over every entry's u32 key length,
                                     key, u32 value length, value
                           u8 recorded; if 1 per entry: u32 length, key,
                                                        u32 length, value
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass, field

import table_golden_io
from table_get_golden_io import patched

MAGIC = b"LGSTSCN1"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_scan.bin")
RECORD_MAX = 64                                     # runs up to this long keep their entries


@dataclass
class Run:
    start: bytes | None
    rc: int
    count: int
    digest: bytes
    entries: list | None                            # [(key, value)] or None


@dataclass
class Case:
    name: str
    set_name: str
    variant: int
    patches: list                                   # [(offset, bytes)]
    internal: int
    bits_per_key: int
    paranoid: int
    verify: int
    open_rc: int = 0
    runs: list = field(default_factory=list)


def table_of(case: Case, sets=None) -> bytes:
    """The case's table image: the named fixture table with its patches."""
    sets = sets if sets is not None else table_golden_io.read()
    s = next(x for x in sets if x.name == case.set_name)
    return patched(s.variants[case.variant].file, case.patches)


def _blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


def _name(s: str) -> bytes:
    e = s.encode()
    return struct.pack("<H", len(e)) + e


def write(path: str, cases: list) -> int:
    out = [MAGIC, struct.pack("<I", len(cases))]
    for c in cases:
        out += [_name(c.name), _name(c.set_name), struct.pack("<II", c.variant, len(c.patches))]
        for off, new in c.patches:
            out += [struct.pack("<I", off), _blob(new)]
        out.append(struct.pack("<BBBBiI", c.internal, c.bits_per_key, c.paranoid, c.verify,
                               c.open_rc, len(c.runs)))
        for r in c.runs:
            assert len(r.digest) == 32
            out += [struct.pack("<B", r.start is not None), _blob(r.start or b""),
                    struct.pack("<iI", r.rc, r.count), r.digest,
                    struct.pack("<B", r.entries is not None)]
            for k, v in r.entries or []:
                out += [_blob(k), _blob(v)]
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH) -> list:
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad table-scan fixture"
    at = 8

    def u(fmt):
        nonlocal at
        r = struct.unpack_from(fmt, data, at)
        at += struct.calcsize(fmt)
        return r

    def blob():
        nonlocal at
        (n,) = u("<I")
        b = data[at:at + n]
        at += n
        return b

    def name():
        nonlocal at
        (n,) = u("<H")
        s = data[at:at + n].decode()
        at += n
        return s

    cases = []
    for _ in range(u("<I")[0]):
        nm, sn = name(), name()
        variant, np_ = u("<II")
        patches = []
        for _ in range(np_):
            (off,) = u("<I")
            patches.append((off, blob()))
        internal, bits, paranoid, verify, open_rc, nr = u("<BBBBiI")
        c = Case(nm, sn, variant, patches, internal, bits, paranoid, verify, open_rc)
        for _ in range(nr):
            (has,) = u("<B")
            start = blob()
            rc, count = u("<iI")
            dg = data[at:at + 32]
            at += 32
            (rec,) = u("<B")
            ents = None
            if rec:
                ents = []
                for _ in range(count):
                    k = blob()
                    ents.append((k, blob()))
            c.runs.append(Run(start if has else None, rc, count, dg, ents))
        cases.append(c)
    assert at == len(data)
    return cases
