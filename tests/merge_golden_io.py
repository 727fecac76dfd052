"""Reader/writer for tests/golden/merge.bin: what lcdb's own merging iterator
delivers over tables, and what its own compactions wrote
(tests/golden/make_merge_golden.py, tests/golden/merge_driver.c).

A run's entries are either a slice of an entry set of
tests/golden/table_build.bin (``set_name``, ``start``, ``stop``, ``step``:
entries[start:stop:step]) or the case's own entries.  An output is recorded
as its count and the SHA-256 over its length-prefixed keys and values
(``digest`` below), and in full when it is short.

The file is one zlib stream of (little-endian):
    magic  b"LGSMRG01"
    u32    merge cases; per case:
        name, u8 internal_keys, u32 runs; per run:
            name ("" = own entries)
            own: u32 entries, then blobs key, value each
            else: u32 start, u32 stop, u32 step
        i32 final status, u32 entries, 32 bytes digest,
        u8 recorded; recorded: blobs key, value per entry
    u32    compaction steps; per step:
        name, u64 smallest_snapshot, u8 drop_deletions,
        u32 block_size, u32 restart_interval, u8 compression, u8 bits_per_key
        u32 input files; per file: blob image, u32 entries, blobs key, value
        blob output image's SHA-256, u32 output bytes,
        u32 entries, blobs key, value
name: u16 length, utf-8; blob: u32 length, bytes.
"""
from __future__ import annotations

import hashlib
import os
import struct
import zlib
from dataclasses import dataclass, field

MAGIC = b"LGSMRG01"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge.bin")
RECORD_MAX = 96                                     # outputs up to this long are kept in full


@dataclass
class Run:
    set_name: str = ""                              # "": own entries
    start: int = 0
    stop: int = 0
    step: int = 1
    own: list = field(default_factory=list)         # [(key, value)]

    def entries(self, sets) -> list:
        if not self.set_name:
            return self.own
        s = next(x for x in sets if x.name == self.set_name)
        return s.entries[self.start:self.stop:self.step]


@dataclass
class MergeCase:
    name: str
    internal: int
    runs: list
    status: int = 0
    count: int = 0
    digest: bytes = b""
    entries: list | None = None                     # None: digest only


@dataclass
class CompactStep:
    name: str
    smallest_snapshot: int
    drop_deletions: int
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    inputs: list                                    # [(image, [(key, value)])]
    out_sha256: bytes = b""
    out_bytes: int = 0
    out_entries: list = field(default_factory=list)


def digest(entries) -> bytes:
    h = hashlib.sha256()
    for k, v in entries:
        h.update(struct.pack("<I", len(k)) + k + struct.pack("<I", len(v)) + v)
    return h.digest()


def _blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


def _name(s: str) -> bytes:
    b = s.encode()
    return struct.pack("<H", len(b)) + b


def _entries(es) -> list:
    out = [struct.pack("<I", len(es))]
    for k, v in es:
        out += [_blob(k), _blob(v)]
    return out


def write(path: str, merges: list, steps: list) -> int:
    out = [MAGIC, struct.pack("<I", len(merges))]
    for c in merges:
        out += [_name(c.name), struct.pack("<BI", c.internal, len(c.runs))]
        for r in c.runs:
            out.append(_name(r.set_name))
            if r.set_name:
                out.append(struct.pack("<III", r.start, r.stop, r.step))
            else:
                out += _entries(r.own)
        out += [struct.pack("<iI", c.status, c.count), c.digest,
                struct.pack("<B", c.entries is not None)]
        if c.entries is not None:
            assert len(c.entries) == c.count
            for k, v in c.entries:
                out += [_blob(k), _blob(v)]
    out.append(struct.pack("<I", len(steps)))
    for s in steps:
        out += [_name(s.name), struct.pack("<QBIIBB", s.smallest_snapshot, s.drop_deletions,
                                           s.block_size, s.restart_interval, s.compression,
                                           s.bits_per_key),
                struct.pack("<I", len(s.inputs))]
        for img, es in s.inputs:
            out += [_blob(img)] + _entries(es)
        out += [_blob(s.out_sha256), struct.pack("<I", s.out_bytes)] + _entries(s.out_entries)
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH):
    """(merge cases, compaction steps)."""
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad merge fixture"
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

    def entries(n=None):
        if n is None:
            (n,) = u("<I")
        out = []
        for _ in range(n):
            k = blob()
            out.append((k, blob()))
        return out

    merges = []
    for _ in range(u("<I")[0]):
        nm = name()
        internal, nruns = u("<BI")
        runs = []
        for _ in range(nruns):
            sn = name()
            runs.append(Run(sn, *u("<III")) if sn else Run(own=entries()))
        status, count = u("<iI")
        dg = data[at:at + 32]
        at += 32
        (rec,) = u("<B")
        merges.append(MergeCase(nm, internal, runs, status, count, dg,
                                entries(count) if rec else None))
    steps = []
    for _ in range(u("<I")[0]):
        nm = name()
        s = CompactStep(nm, *u("<QBIIBB"), [])
        for _ in range(u("<I")[0]):
            img = blob()
            s.inputs.append((img, entries()))
        s.out_sha256 = blob()
        (s.out_bytes,) = u("<I")
        s.out_entries = entries()
        steps.append(s)
    assert at == len(data)
    return merges, steps
