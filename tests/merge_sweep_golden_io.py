"""Reader/writer for tests/golden/merge_sweep.bin: what lcdb's own compaction
loop kept and wrote, and what its own merging iterator delivered, for every
case of tests/merge_sweep.py (tests/golden/make_merge_sweep_golden.py,
merge_driver.c).

No inputs are kept: a case's sources are regenerated (merge_sweep.sources,
merge_sweep.tables) and checked against the recorded counts and digests.  An
output is recorded as its count and digest (merge_golden_io.digest), in full
when it has at most RECORD_MAX entries, and the file lcdb wrote as its size
and SHA-256.

The file is one zlib stream of (little-endian):
    magic  b"LGSMSW01"
    u32    cases; per case:
        name, u8 kind (0 repair, 1 wide),
        u32 sources; per source: name, u32 entries, 32 bytes digest
        kind 0: u32 steps; per step:
            name, u32 inputs; per input: the source's name, in the order lcdb
            handed the files to its merging iterator ("o0": the first step's output)
            u64 smallest_snapshot, u8 drop_deletions,
            u32 kept entries, 32 bytes digest, u8 recorded; recorded: blobs key, value each
            u8 file written; written: u32 bytes, 32 bytes SHA-256
        kind 1: u32 merged entries, 32 bytes digest, u8 recorded; recorded: blobs
name: u16 length, utf-8; blob: u32 length, bytes.
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass, field

from merge_golden_io import RECORD_MAX, digest  # noqa: F401  (re-exported)

MAGIC = b"LGSMSW01"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_sweep.bin")
KINDS = ("repair", "wide")


@dataclass
class Step:
    name: str
    inputs: list                                    # source names, lcdb's order
    smallest_snapshot: int
    drop_deletions: int
    count: int = 0
    digest: bytes = b""
    entries: list | None = None                     # None: digest only
    out_bytes: int | None = None                    # None: lcdb wrote no file
    out_sha256: bytes = b""


@dataclass
class Record:
    name: str
    kind: str
    sources: list = field(default_factory=list)     # [(name, entries, digest)]
    steps: list = field(default_factory=list)       # repair
    count: int = 0                                  # wide: the merged order
    digest: bytes = b""
    entries: list | None = None


def _name(s: str) -> bytes:
    b = s.encode()
    return struct.pack("<H", len(b)) + b


def _blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


def _kept(count, dg, entries) -> list:
    out = [struct.pack("<I", count), dg, struct.pack("<B", entries is not None)]
    if entries is not None:
        assert len(entries) == count
        for k, v in entries:
            out += [_blob(k), _blob(v)]
    return out


def write(path: str, records: list) -> int:
    out = [MAGIC, struct.pack("<I", len(records))]
    for r in records:
        out += [_name(r.name), struct.pack("<BI", KINDS.index(r.kind), len(r.sources))]
        for nm, n, dg in r.sources:
            out += [_name(nm), struct.pack("<I", n), dg]
        if r.kind == "wide":
            out += _kept(r.count, r.digest, r.entries)
            continue
        out.append(struct.pack("<I", len(r.steps)))
        for s in r.steps:
            out += [_name(s.name), struct.pack("<I", len(s.inputs))] + [_name(i) for i in s.inputs]
            out.append(struct.pack("<QB", s.smallest_snapshot, s.drop_deletions))
            out += _kept(s.count, s.digest, s.entries)
            out.append(struct.pack("<B", s.out_bytes is not None))
            if s.out_bytes is not None:
                out += [struct.pack("<I", s.out_bytes), s.out_sha256]
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH) -> list:
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad merge sweep fixture"
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

    def kept():
        (n,) = u("<I")
        dg = raw(32)
        es = None
        if u("<B")[0]:
            es = []
            for _ in range(n):
                k = raw(u("<I")[0])
                es.append((k, raw(u("<I")[0])))
        return n, dg, es

    out = []
    for _ in range(u("<I")[0]):
        nm = name()
        kind, nsrc = u("<BI")
        r = Record(nm, KINDS[kind])
        for _ in range(nsrc):
            sn = name()
            r.sources.append((sn, u("<I")[0], raw(32)))
        if r.kind == "wide":
            r.count, r.digest, r.entries = kept()
        else:
            for _ in range(u("<I")[0]):
                sn = name()
                inputs = [name() for _ in range(u("<I")[0])]
                s = Step(sn, inputs, *u("<QB"))
                s.count, s.digest, s.entries = kept()
                if u("<B")[0]:
                    (s.out_bytes,) = u("<I")
                    s.out_sha256 = raw(32)
                r.steps.append(s)
        out.append(r)
    assert at == len(data)
    return out
