"""Reader/writer for tests/golden/compact_version.bin: what lcdb's compaction
loop writes inside a version, with ldb_compaction_should_stop_before and
ldb_compaction_is_base_level_for_key at work (tests/golden/
make_version_golden.py, tests/golden/version_driver.c).

A loop case is an already merged entry list, the file lists of levels
output + 1 .. 6 (level + 2 first) and the loop's parameters, with what lcdb's
own functions answered per entry (bit 0: should_stop_before returned 1, bit 1:
the entry was dropped) and the files its table builder wrote.  The compaction
is one real lcdb compaction of a level-0 and a level-1 table over a populated
level 2: the input tables whole, newest first as ldb_inputiter_create orders
them, level 2 as (smallest, largest, size), and the output files.

The file is one zlib stream of (little-endian):
    magic  b"LGSVER01"
    u32    loop cases; per case:
        name, u32 block_size, u32 restart_interval, u8 compression,
        u8 bits_per_key, u64 max_output_file_size, u64 max_file_size option
        (the limit is 10 x that), u64 smallest_snapshot
        levels
        u32 entries; per entry blobs key, value
        per entry u8 flags
        files
    u8     a compaction follows (0 or 1):
        u32 block_size, u32 restart_interval, u8 compression, u8 bits_per_key,
        u64 max_output_file_size, u64 max_file_size option, u64 smallest_snapshot
        levels
        u32 input tables; per table blob image
        files
levels: u8 count; per level u32 files; per file blobs smallest, largest, u64 size.
files:  u32 count; per file: u32 entries, u32 bytes, 32 bytes SHA-256, blobs
        smallest key, largest key, u8 image follows, blob image.
name: u16 length, utf-8; blob: u32 length, bytes.
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass, field

from split_golden_io import OutFile, out_file  # noqa: F401  (the same file record)

MAGIC = b"LGSVER01"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compact_version.bin")
STOP, DROP = 1, 2


@dataclass
class LoopCase:
    name: str
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    max_output_file_size: int
    max_file_size: int                  # the option: max_grandparent_overlap_bytes = 10 x this
    smallest_snapshot: int
    levels: list = field(default_factory=list)      # [[(smallest, largest, size)]], level + 2 first
    entries: list = field(default_factory=list)     # merged order, before the drop rule
    flags: bytes = b""                  # per entry: STOP | DROP as lcdb answered
    files: list = field(default_factory=list)

    @property
    def limit(self) -> int:
        return 10 * self.max_file_size

    def kept(self) -> list:
        return [e for e, f in zip(self.entries, self.flags) if not f & DROP]

    def file_first(self) -> list:
        out = [0]
        for f in self.files:
            out.append(out[-1] + f.entries)
        return out


@dataclass
class Compaction:
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    max_output_file_size: int
    max_file_size: int
    smallest_snapshot: int
    levels: list = field(default_factory=list)
    inputs: list = field(default_factory=list)      # table images, newest level-0 file first
    files: list = field(default_factory=list)

    @property
    def limit(self) -> int:
        return 10 * self.max_file_size


def _blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


def _name(s: str) -> bytes:
    b = s.encode()
    return struct.pack("<H", len(b)) + b


def _levels(levels) -> list:
    out = [struct.pack("<B", len(levels))]
    for files in levels:
        out.append(struct.pack("<I", len(files)))
        for lo, hi, size in files:
            out += [_blob(lo), _blob(hi), struct.pack("<Q", size)]
    return out


def _files(files) -> list:
    out = [struct.pack("<I", len(files))]
    for f in files:
        out += [struct.pack("<II", f.entries, f.size), f.sha256, _blob(f.smallest), _blob(f.largest),
                struct.pack("<B", f.image is not None), _blob(f.image or b"")]
    return out


def write(path: str, cases: list, compact: Compaction | None) -> int:
    out = [MAGIC, struct.pack("<I", len(cases))]
    for c in cases:
        out += [_name(c.name),
                struct.pack("<IIBBQQQ", c.block_size, c.restart_interval, c.compression,
                            c.bits_per_key, c.max_output_file_size, c.max_file_size,
                            c.smallest_snapshot)]
        out += _levels(c.levels)
        out.append(struct.pack("<I", len(c.entries)))
        for k, v in c.entries:
            out += [_blob(k), _blob(v)]
        assert len(c.flags) == len(c.entries)
        out.append(bytes(c.flags))
        out += _files(c.files)
    out.append(struct.pack("<B", compact is not None))
    if compact is not None:
        c = compact
        out.append(struct.pack("<IIBBQQQ", c.block_size, c.restart_interval, c.compression,
                               c.bits_per_key, c.max_output_file_size, c.max_file_size,
                               c.smallest_snapshot))
        out += _levels(c.levels)
        out.append(struct.pack("<I", len(c.inputs)))
        out += [_blob(img) for img in c.inputs]
        out += _files(c.files)
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH):
    """(loop cases, the compaction or None)."""
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad version fixture"
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

    def blob():
        return raw(u("<I")[0])

    def levels():
        out = []
        for _ in range(u("<B")[0]):
            files = []
            for _ in range(u("<I")[0]):
                lo, hi = blob(), blob()
                files.append((lo, hi, u("<Q")[0]))
            out.append(files)
        return out

    def files():
        out = []
        for _ in range(u("<I")[0]):
            n, size = u("<II")
            sha, lo, hi = raw(32), blob(), blob()
            (keep,) = u("<B")
            img = blob()
            out.append(OutFile(n, size, sha, lo, hi, img if keep else None))
        return out

    cases = []
    for _ in range(u("<I")[0]):
        c = LoopCase(raw(u("<H")[0]).decode(), *u("<IIBBQQQ"))
        c.levels = levels()
        for _ in range(u("<I")[0]):
            k = blob()
            c.entries.append((k, blob()))
        c.flags = raw(len(c.entries))
        c.files = files()
        cases.append(c)
    compact = None
    if u("<B")[0]:
        compact = Compaction(*u("<IIBBQQQ"))
        compact.levels = levels()
        compact.inputs = [blob() for _ in range(u("<I")[0])]
        compact.files = files()
    assert at == len(data)
    return cases, compact
