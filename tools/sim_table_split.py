#!/usr/bin/env python3
"""Compaction's output files, serial and as block boundaries.

Serial rule (the reference restated): for every kept entry the compaction
opens an output table if none is open, adds the entry, and closes the table
once ldb_tablegen_size has reached max_output_file_size (db_impl.c:1399-1425);
the table builder is table_builder.c:215-365 (`TableGen` below, over
sim_block_cut's block builder and the oracle's block framing and filter
block).

Block-boundary formulation (what lgs_tables_build_dev runs):
ldb_tablegen_size is the builder's offset (table_builder.c:384-386), which
moves only when a block is flushed, and before ldb_tablegen_finish a flush
happens only in ldb_tablegen_add behind the entry that filled the block
(:251-254).  So for max_output_file_size >= 1 a file ends directly after a
block flush, with no block pending:
  1. the data blocks of all files are the blocks of one cut over all entries,
     framed once from offset 0: start[b], end[b] = start[b] + size[b] + 5;
  2. a file that starts at block s ends after the first block b >= s with
     end[b] - start[s] >= max_output_file_size (monotone in b: a search);
  3. the file starts are what that relation reaches from block 0;
  4. per file only the handles (offsets from start[s]), the last block's
     index key (the short successor, :332-341), the filter block, the
     metaindex, the index block and the footer are the file's own.

usage: python tools/sim_table_split.py [SETS]      (seeded random entry sets)
"""
from __future__ import annotations

import os
import random
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sim_block_cut import RESTARTS, BlockGen, random_entries, separator, serial_blocks, successor, varint  # noqa: E402

FILTER_KEY = b"filter.leveldb.BuiltinBloomFilter2"
MAGIC = 0xdb4775248b80fb57                                       # format.h:26
NO_SPLIT = (1 << 64) - 1


def handle(off: int, size: int) -> bytes:                        # format.c:45-63
    return varint(off) + varint(size)


class TableGen:
    """table_builder.c:70-386 for one output file."""

    def __init__(self, block_size: int, restart_interval: int, compression: int,
                 bits_per_key: int, internal: bool):
        import oracle
        self.oracle = oracle
        self.block_size, self.R, self.compression = block_size, restart_interval, compression
        self.bits, self.internal = bits_per_key, internal
        self.data = BlockGen(restart_interval)
        self.index = BlockGen(1)                                 # :87
        self.file = bytearray()
        self.entries = 0
        self.last_key = b""
        self.pending = None                                      # the flushed block's handle
        self.block_keys, self.block_offs, self.keys = [], [], []  # the filter block's input

    def size(self) -> int:                                       # :384-386
        return len(self.file)

    def write_block(self, raw: bytes, compression: int):         # :123-213
        region, hoff, hsize, end = self.oracle.table_write_blocks([raw], compression, len(self.file))
        self.file += region
        assert end == len(self.file)
        return int(hoff[0]), int(hsize[0])

    def add(self, key: bytes, value: bytes):                     # :215-255
        if self.pending is not None:
            self.index.add(separator(self.last_key, key, self.internal), handle(*self.pending))
            self.pending = None
        self.keys.append(key)
        self.last_key = key
        self.entries += 1
        self.data.add(key, value)
        if self.data.estimate() >= self.block_size:
            self.flush()

    def flush(self):                                             # :257-278
        if self.data.empty():
            return
        self.block_offs.append(len(self.file))
        self.block_keys.append(self.keys)
        self.keys = []
        self.pending = self.write_block(self.data.finish(), self.compression)
        self.data.reset()

    def finish(self) -> bytes:                                   # :280-365
        self.flush()
        meta = BlockGen(self.R)
        if self.bits > 0:
            fb = self.oracle.bloom_restatement().filter_block(
                self.block_keys, self.block_offs, len(self.file), self.bits, self.internal)
            meta.add(FILTER_KEY, handle(*self.write_block(fb, 0)))
        meta_handle = self.write_block(meta.finish(), self.compression)
        if self.pending is not None:
            self.index.add(successor(self.last_key, self.internal), handle(*self.pending))
            self.pending = None
        index_handle = self.write_block(self.index.finish(), self.compression)
        footer = handle(*meta_handle) + handle(*index_handle)    # format.c:92-106
        self.file += footer + b"\0" * (40 - len(footer)) + struct.pack("<Q", MAGIC)
        return bytes(self.file)


def split_serial(entries, block_size: int = 4096, restart_interval: int = 16, compression: int = 0,
                 bits_per_key: int = 0, internal: bool = False, max_file_size: int = NO_SPLIT):
    """(file_first with files + 1 values, file images): db_impl.c:1399-1425
    over entries the drop rule kept."""
    assert max_file_size >= 1
    first, images, gen = [], [], None
    for i, (k, v) in enumerate(entries):
        if gen is None:                                          # :1401-1406
            gen = TableGen(block_size, restart_interval, compression, bits_per_key, internal)
            first.append(i)
        gen.add(k, v)                                            # :1415
        if gen.size() >= max_file_size:                          # :1418-1424
            images.append(gen.finish())
            gen = None
    if gen is not None:                                          # :1433-1434
        images.append(gen.finish())
    return first + [len(entries)], images


def split_blocks(entries, block_size: int, restart_interval: int, compression: int,
                 max_file_size: int):
    """file_first by steps 1-3 of the block-boundary formulation."""
    import oracle
    bfirst, blocks = serial_blocks(entries, block_size, restart_interval)
    nb = len(blocks)
    if nb == 0:
        return [0]
    _, hoff, hsize, _ = oracle.table_write_blocks(blocks, compression, 0)
    start = [int(x) for x in hoff]
    end = [int(o) + int(s) + 5 for o, s in zip(hoff, hsize)]
    nxt = []
    for s in range(nb):
        lo, hi = s, nb                                           # first b with the size reached
        while lo < hi:
            mid = (lo + hi) // 2
            if end[mid] - start[s] >= max_file_size:
                hi = mid
            else:
                lo = mid + 1
        nxt.append(min(lo + 1, nb))
    nxt.append(nb)
    mark = [False] * (nb + 1)
    mark[0] = True
    jump = nxt
    for _ in range(max(1, nb.bit_length())):                     # pointer doubling
        for s in range(nb):
            if mark[s]:
                mark[jump[s]] = True
        jump = [jump[j] for j in jump]
    return [bfirst[b] for b in range(nb) if mark[b]] + [len(entries)]


def main() -> None:
    sets = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    rng = random.Random(20249)
    files = 0
    for t in range(sets):
        n = rng.choice([1, 2, 17, 100, 400])
        e = random_entries(rng, n)
        bs = rng.choice([1, 64, 256, 1024])
        R = rng.choice(RESTARTS)
        comp = rng.choice([0, 1])
        mx = rng.choice([1, 100, 300, 1024, 5000, NO_SPLIT])
        want, images = split_serial(e, bs, R, comp, rng.choice([0, 10]), False, mx)
        assert split_blocks(e, bs, R, comp, mx) == want, (t, n, bs, R, mx)
        files += len(images)
    print(f"{sets} entry sets, {files} files: the block-boundary split equals the serial rule")


if __name__ == "__main__":
    main()
