"""Reader/writer for tests/golden/table_build.bin: tables written by lcdb's own
ldb_tablegen_* (tests/golden/make_table_golden.py) with the entries and
options that produced them.

The file is one zlib stream of (little-endian):
    magic  b"LGSTBLD1"
    u32    entry sets
    per set:
        u16 name length, name (utf-8)
        u32 entries; per entry: u32 key length, key, u32 value length, value
        u32 variants; per variant:
            u32 block_size, u32 restart_interval, u8 compression,
            u8 bits_per_key, u8 internal_keys
            u32 length, the .ldb file
            u32 data blocks; per block: u32 length, raw contents
                                        u32 length, its index key
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass, field

MAGIC = b"LGSTBLD1"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_build.bin")


@dataclass
class Variant:
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    internal: int
    file: bytes = b""
    blocks: list = field(default_factory=list)      # raw data blocks
    ikeys: list = field(default_factory=list)       # the index block's keys


@dataclass
class EntrySet:
    name: str
    entries: list                                   # [(key, value)]
    variants: list


def _blob(b: bytes) -> bytes:
    return struct.pack("<I", len(b)) + b


def write(path: str, sets: list) -> int:
    out = [MAGIC, struct.pack("<I", len(sets))]
    for s in sets:
        nm = s.name.encode()
        out += [struct.pack("<H", len(nm)), nm, struct.pack("<I", len(s.entries))]
        for k, v in s.entries:
            out += [_blob(k), _blob(v)]
        out.append(struct.pack("<I", len(s.variants)))
        for v in s.variants:
            out.append(struct.pack("<IIBBB", v.block_size, v.restart_interval, v.compression,
                                   v.bits_per_key, v.internal))
            out += [_blob(v.file), struct.pack("<I", len(v.blocks))]
            for b, k in zip(v.blocks, v.ikeys):
                out += [_blob(b), _blob(k)]
    data = zlib.compress(b"".join(out), 9)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read(path: str = PATH) -> list:
    with open(path, "rb") as f:
        data = zlib.decompress(f.read())
    assert data[:8] == MAGIC, "bad table fixture"
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

    sets = []
    for _ in range(u("<I")[0]):
        (nl,) = u("<H")
        name = data[at:at + nl].decode()
        at += nl
        entries = []
        for _ in range(u("<I")[0]):
            k = blob()
            entries.append((k, blob()))
        variants = []
        for _ in range(u("<I")[0]):
            v = Variant(*u("<IIBBB"))
            v.file = blob()
            for _ in range(u("<I")[0]):
                v.blocks.append(blob())
                v.ikeys.append(blob())
            variants.append(v)
        sets.append(EntrySet(name, entries, variants))
    return sets
