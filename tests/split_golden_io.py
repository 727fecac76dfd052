"""Reader/writer for tests/golden/compact_split.bin: the files lcdb's own
table builder writes when it is driven as a compaction drives it, with an
arbitrary max_output_file_size, and the output files of one real lcdb
compaction (tests/golden/make_split_golden.py, tests/golden/split_driver.c).

A split case's entries are an entry set of tests/golden/table_build.bin
(``source`` = its name), generated (``source`` = "gen:<n>:<step>:<internal>",
``gen_entries`` below) or the case's own (``source`` = "", recorded in full).
The compaction's inputs are generated (``compact_inputs`` below) and recorded
as each level-0 table's SHA-256 and entry count.  An output file is recorded
as its entry count, size, SHA-256 and first and last key, and as its image
when the case's images are small.

The file is one zlib stream of (little-endian):
    magic  b"LGSSPL01"
    u32    split cases; per case:
        name, source, u32 block_size, u32 restart_interval, u8 compression,
        u8 bits_per_key, u8 internal_keys, u64 max_file_size,
        u32 entries, 32 bytes digest of the entries (merge_golden_io.digest),
        own entries (source ""): blobs key, value per entry
        files
    u8     a compaction follows (0 or 1):
        u32 level-0 files, u32 user keys, u64 smallest_snapshot,
        u8 drop_deletions, u32 block_size, u32 restart_interval,
        u8 compression, u8 bits_per_key, u64 max_file_size
        per level-0 file, oldest first: u32 entries, 32 bytes SHA-256 of the table
        files
files: u32 count; per file: u32 entries, u32 bytes, 32 bytes SHA-256,
       blobs smallest key, largest key, u8 image follows, blob image.
name, source: u16 length, utf-8; blob: u32 length, bytes.
"""
from __future__ import annotations

import hashlib
import os
import struct
import zlib
from dataclasses import dataclass, field

from merge_golden_io import digest  # noqa: F401  (re-exported: the entry stream's digest)

MAGIC = b"LGSSPL01"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compact_split.bin")
NO_SPLIT = (1 << 64) - 1


@dataclass
class OutFile:
    entries: int
    size: int
    sha256: bytes
    smallest: bytes
    largest: bytes
    image: bytes | None = None


@dataclass
class SplitCase:
    name: str
    source: str
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    internal: int
    max_file_size: int
    count: int = 0
    digest: bytes = b""
    own: list = field(default_factory=list)
    files: list = field(default_factory=list)

    def entries(self, sets) -> list:
        if not self.source:
            return self.own
        if self.source.startswith("gen:"):
            return gen_entries(*(int(x) for x in self.source.split(":")[1:]))
        return next(s for s in sets if s.name == self.source).entries


@dataclass
class CompactCase:
    l0_files: int
    user_keys: int
    smallest_snapshot: int
    drop_deletions: int
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    max_file_size: int
    inputs: list = field(default_factory=list)      # [(entries, SHA-256 of the table)], oldest first
    files: list = field(default_factory=list)


def tag(seq: int, typ: int) -> bytes:               # dbformat.h: pack_seqtype, fixed64
    return struct.pack("<Q", (seq << 8) | typ)


def gen_entries(n: int, step: int, internal: int) -> list:
    """n entries of 16 + 32 bytes (internal keys: 8 more), keys increasing."""
    out = []
    for i in range(n):
        k = b"%016d" % (i * step)
        if internal:
            k += tag(1000 + i, 1)
        out.append((k, (b"%08x" % (i * 2654435761 & 0xffffffff)) * 4))
    return out


def compact_ops(l0_files: int, user_keys: int) -> list:
    """The writes of the compaction case, one list per level-0 file (oldest
    first): ("p", user key, value) or ("d", user key).  File j rewrites a
    share of the keys of the files before it and deletes a few of them."""
    files = []
    for j in range(l0_files):
        ops = []
        for i in range(user_keys):
            if i % l0_files == j or (j and i % 11 == j):
                ops.append(("p", b"user%012d" % i, (b"%08d.%d/" % (i, j)) * 9))
            elif j and i % 61 == 7 * j:
                ops.append(("d", b"user%012d" % i))
        files.append(ops)
    return files


def compact_inputs(l0_files: int, user_keys: int):
    """([[(internal key, value)] per level-0 file, oldest first], last
    sequence): a write takes the next sequence, and a flushed memtable is in
    internal-key order (user key up, sequence down)."""
    seq, out = 0, []
    for ops in compact_ops(l0_files, user_keys):
        es = []
        for op in ops:
            seq += 1
            es.append((op[1], seq, 1 if op[0] == "p" else 0, op[2] if op[0] == "p" else b""))
        es.sort(key=lambda e: (e[0], -e[1]))
        out.append([(u + tag(s, t), v) for u, s, t, v in es])
    return out, seq


def _blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


def _name(s: str) -> bytes:
    b = s.encode()
    return struct.pack("<H", len(b)) + b


def _files(files) -> list:
    out = [struct.pack("<I", len(files))]
    for f in files:
        out += [struct.pack("<II", f.entries, f.size), f.sha256, _blob(f.smallest), _blob(f.largest),
                struct.pack("<B", f.image is not None), _blob(f.image or b"")]
    return out


def out_file(entries, image: bytes, keep: bool) -> OutFile:
    return OutFile(len(entries), len(image), hashlib.sha256(image).digest(), entries[0][0],
                   entries[-1][0], image if keep else None)


def write(path: str, cases: list, compact: CompactCase | None) -> int:
    out = [MAGIC, struct.pack("<I", len(cases))]
    for c in cases:
        out += [_name(c.name), _name(c.source),
                struct.pack("<IIBBBQ", c.block_size, c.restart_interval, c.compression,
                            c.bits_per_key, c.internal, c.max_file_size),
                struct.pack("<I", c.count), c.digest]
        if not c.source:
            assert len(c.own) == c.count
            for k, v in c.own:
                out += [_blob(k), _blob(v)]
        out += _files(c.files)
    out.append(struct.pack("<B", compact is not None))
    if compact is not None:
        c = compact
        out.append(struct.pack("<IIQBIIBBQ", c.l0_files, c.user_keys, c.smallest_snapshot,
                               c.drop_deletions, c.block_size, c.restart_interval, c.compression,
                               c.bits_per_key, c.max_file_size))
        assert len(c.inputs) == c.l0_files
        for n, sha in c.inputs:
            out += [struct.pack("<I", n), sha]
        out += _files(c.files)
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH):
    """(split cases, the compaction case or None)."""
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad split fixture"
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

    def name():
        return raw(u("<H")[0]).decode()

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
        c = SplitCase(name(), name(), *u("<IIBBBQ"))
        (c.count,) = u("<I")
        c.digest = raw(32)
        if not c.source:
            for _ in range(c.count):
                k = blob()
                c.own.append((k, blob()))
        c.files = files()
        cases.append(c)
    compact = None
    if u("<B")[0]:
        compact = CompactCase(*u("<IIQBIIBBQ"))
        for _ in range(compact.l0_files):
            (n,) = u("<I")
            compact.inputs.append((n, raw(32)))
        compact.files = files()
    assert at == len(data)
    return cases, compact
