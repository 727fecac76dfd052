"""Reader/writer for tests/golden/read_sweep.bin: what lcdb's own table
reader returned for the targets and scan starts of every table of
tests/read_sweep.py (tests/golden/make_read_sweep_golden.py).

No keys, values or images are kept.  A table's entries, image, targets and
starts are regenerated (read_sweep.py); an outcome names an entry by its
ordinal in the table's entries, since the recipe has asserted that lcdb's key
and value bytes are that entry's, and a scan by the ordinal of its first entry,
since the recipe has asserted that lcdb delivered entries[ordinal:].

The file is one zlib stream of (little-endian):
    magic  b"LGSRSW01"
    u32    tables; per table:
        name, case (u16 length, utf-8), u32 file number,
        i32 rc of ldb_table_open,
        u8 versions; if set: u32 entries, 32 bytes digest of the entry set,
                             u32 bytes, 32 bytes SHA-256 of lcdb's file,
        u32 targets; then column by column:
            i32 rc of ldb_table_internal_get per target,
            u8 flags per target: 1 = handle_result was called; 2 = it was not,
               but is when the same file is read without its filter policy,
            u16 ordinal per target (0xffff: not called),
        u32 starts; per start: i32 final ldb_iter_status, u32 entries
                    delivered, u32 ordinal of the first (the entry count: none).
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass, field

MAGIC = b"LGSRSW01"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_sweep.bin")
CALLED, REFUSED = 1, 2
NONE = 0xffff


@dataclass
class Record:
    name: str
    case: str
    file: int
    open_rc: int = 0
    count: int = 0                                   # versions tables only: the entry set
    digest: bytes = b""
    size: int = 0                                    # ... and lcdb's file
    sha: bytes = b""
    rc: list = field(default_factory=list)           # per target
    flags: list = field(default_factory=list)
    ordinal: list = field(default_factory=list)
    starts: list = field(default_factory=list)       # [(rc, count, ordinal)]


def _name(s: str) -> bytes:
    b = s.encode()
    return struct.pack("<H", len(b)) + b


def write(path: str, records: list) -> int:
    out = [MAGIC, struct.pack("<I", len(records))]
    for r in records:
        n = len(r.rc)
        assert len(r.flags) == n and len(r.ordinal) == n
        out += [_name(r.name), _name(r.case), struct.pack("<IiB", r.file, r.open_rc, bool(r.sha))]
        if r.sha:
            out += [struct.pack("<I", r.count), r.digest, struct.pack("<I", r.size), r.sha]
        out += [struct.pack("<I", n), struct.pack(f"<{n}i", *r.rc), bytes(r.flags),
                struct.pack(f"<{n}H", *r.ordinal), struct.pack("<I", len(r.starts))]
        out += [struct.pack("<iII", *s) for s in r.starts]
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH) -> list:
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad read sweep fixture"
    at = 8

    def u(fmt):
        nonlocal at
        r = struct.unpack_from(fmt, data, at)
        at += struct.calcsize(fmt)
        return r

    def raw(n):
        nonlocal at
        b = data[at:at + n]
        at += n
        return b

    def name():
        return raw(u("<H")[0]).decode()

    out = []
    for _ in range(u("<I")[0]):
        r = Record(name(), name(), *u("<Ii"))
        if u("<B")[0]:
            (r.count,) = u("<I")
            r.digest = raw(32)
            (r.size,) = u("<I")
            r.sha = raw(32)
        (n,) = u("<I")
        r.rc = list(u(f"<{n}i"))
        r.flags = list(raw(n))
        r.ordinal = list(u(f"<{n}H"))
        r.starts = [u("<iII") for _ in range(u("<I")[0])]
        out.append(r)
    assert at == len(data)
    return out
