"""Reader/writer for tests/golden/build_sweep.bin: what lcdb's own table
builder wrote for every case of tests/build_sweep.py, driven as a compaction
drives it (tests/golden/make_build_sweep_golden.py, split_driver.c).

No entries and no images are kept: an entry set is regenerated from its spec
(build_sweep.entries) and checked against the recorded count and digest, and
an output file is recorded as its entry count, size and SHA-256.

The file is one zlib stream of (little-endian):
    magic  b"LGSSWP01"
    u32    cases; per case:
        name, spec (u16 length, utf-8),
        u32 block_size, u32 restart_interval, u8 compression, u8 bits_per_key,
        u8 internal_keys, u64 max_file_size,
        u32 entries, 32 bytes digest of the entries (merge_golden_io.digest),
        u32 files; per file: u32 entries, u32 bytes, 32 bytes SHA-256.
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass, field

from merge_golden_io import digest  # noqa: F401  (re-exported: the entry stream's digest)

MAGIC = b"LGSSWP01"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_sweep.bin")


@dataclass
class Record:
    name: str
    spec: str
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    internal: int
    max_file_size: int
    count: int = 0
    digest: bytes = b""
    files: list = field(default_factory=list)       # [(entries, bytes, SHA-256)]

    def options(self):
        return (self.block_size, self.restart_interval, self.compression, self.bits_per_key,
                self.internal, self.max_file_size)


def _name(s: str) -> bytes:
    b = s.encode()
    return struct.pack("<H", len(b)) + b


def write(path: str, records: list) -> int:
    out = [MAGIC, struct.pack("<I", len(records))]
    for r in records:
        out += [_name(r.name), _name(r.spec),
                struct.pack("<IIBBBQ", r.block_size, r.restart_interval, r.compression,
                            r.bits_per_key, r.internal, r.max_file_size),
                struct.pack("<I", r.count), r.digest, struct.pack("<I", len(r.files))]
        for n, size, sha in r.files:
            out += [struct.pack("<II", n, size), sha]
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH) -> list:
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad build sweep fixture"
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
        r = Record(name(), name(), *u("<IIBBBQ"))
        (r.count,) = u("<I")
        r.digest = raw(32)
        for _ in range(u("<I")[0]):
            n, size = u("<II")
            r.files.append((n, size, raw(32)))
        out.append(r)
    assert at == len(data)
    return out
