"""Reader/writer for tests/golden/table_get.bin: what lcdb's own
ldb_table_internal_get returned for point lookups in the tables of
tests/golden/table_build.bin (tests/golden/make_get_golden.py).

A case names its table by entry set and variant index of table_build.bin and
does not repeat its bytes; a patched table is the list of (offset, new bytes)
applied to it.  The file is one zlib stream of (little-endian):
    magic  b"LGSTGET1"
    u32    cases
    per case:
        u16 name length, name (utf-8)             -- what the case is about
        u16 set name length, set name; u32 variant index
        u32 patches; per patch: u32 offset, u32 length, bytes
        u8 internal_keys, u8 bits_per_key, u8 paranoid_checks, u8 verify_checksums
        i32 rc of ldb_table_open
        u32 queries; per query: u32 length, key
                                i32 rc, u8 called
                                u32 length, found key; u32 length, found value
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass, field

import table_golden_io

MAGIC = b"LGSTGET1"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_get.bin")


@dataclass
class Record:
    key: bytes
    rc: int
    called: int
    found_key: bytes
    found_value: bytes


@dataclass
class Case:
    name: str
    set_name: str
    variant: int
    patches: list                                    # [(offset, bytes)]
    internal: int
    bits_per_key: int
    paranoid: int
    verify: int
    open_rc: int = 0
    records: list = field(default_factory=list)


def patched(file: bytes, patches) -> bytes:
    b = bytearray(file)
    for off, new in patches:
        b[off:off + len(new)] = new
    assert len(b) == len(file)
    return bytes(b)


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
                               c.open_rc, len(c.records)))
        for r in c.records:
            out += [_blob(r.key), struct.pack("<iB", r.rc, r.called), _blob(r.found_key),
                    _blob(r.found_value)]
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH) -> list:
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad table-get fixture"
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
        internal, bits, paranoid, verify, open_rc, nq = u("<BBBBiI")
        c = Case(nm, sn, variant, patches, internal, bits, paranoid, verify, open_rc)
        for _ in range(nq):
            k = blob()
            rc, called = u("<iB")
            fk = blob()
            c.records.append(Record(k, rc, called, fk, blob()))
        cases.append(c)
    return cases


def version_entries() -> list:
    """Hand-made internal-key entries no fixture table has in one block: many
    versions of one user key, whose tags share leading bytes, so that an entry's
    `shared` count reaches into the previous key's tag (dbformat.c:206-230
    sorts the larger sequence first).  Checked against the Python model only;
    the `versions` family of tests/read_sweep.py is what holds these shapes
    to lcdb (tests/golden/read_sweep.bin)."""
    def ik(user, seq, typ=1):
        return user + struct.pack("<Q", (seq << 8) | typ)
    seqs = [0x060403, 0x050403, 0x050402, 0x040402, 0x030402, 0x000402, 0x000302]
    e = [(ik(b"u", 0x070403), b"first")]
    e += [(ik(b"v", s, i % 2), b"val%d" % i) for i, s in enumerate(seqs)]
    e += [(ik(b"v\x01\x03", 0x0403), b"longer"), (ik(b"vv", 0x050403), b"vv"), (ik(b"w", 1), b"")]
    return e
