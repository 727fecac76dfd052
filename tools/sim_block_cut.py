#!/usr/bin/env python3
"""The data-block cut of lcdb's table builder, serial and parallel.

Serial rule (the reference restated): ldb_tablegen_add (table_builder.c:215-255)
feeds every entry to ldb_blockgen_add (block_builder.c:91-136) and flushes the
block once ldb_blockgen_size_estimate (:153-158) reaches block_size; the index
key of a block is the comparator's shortest separator of its last key and the
next block's first key, the short successor of the last key for the last block
(comparator.c:44-88, dbformat.c:232-285).

Parallel formulation (what lgs_block.hip runs):
  1. lcp[i] = common prefix of keys i-1 and i;
     sh[i] = vl(lcp) + vl(klen-lcp) + vl(vlen) + (klen-lcp) + vlen,
     fu[i] = 1 + vl(klen) + vl(vlen) + klen + vlen   (entry at a restart);
  2. S = prefix sum of sh; C[i] = (fu[i]-sh[i]) + C[i-R]  (stride-R prefix);
  3. a block from s to j (m = j-s+1 entries) has the estimate
       S[j+1]-S[s] + C[s + (j-s)//R*R] - C[s-R] + 4*ceil(m/R) + 4,
     monotone in j, so next[s] is a binary search;
  4. the block starts are the entries reachable from 0 through next[]:
     ceil(log2(n+1)) rounds of  mark[J[s]] = 1 for marked s;  J = J o J.

usage: python tools/sim_block_cut.py [SETS]      (seeded random entry sets)
"""
from __future__ import annotations

import random
import struct
import sys

RESTARTS = [1, 2, 3, 5, 7, 16, 17, 64]            # the self-checks' restart intervals (tests/build_sweep.py)
MAX_SEQ_SEEK = ((((1 << 56) - 1) << 8) | 1).to_bytes(8, "little")   # dbformat.h: pack_seqtype


def varint(x: int) -> bytes:
    out = bytearray()
    while x >= 128:
        out.append((x & 127) | 128)
        x >>= 7
    out.append(x)
    return bytes(out)


def vl(x: int) -> int:
    return 1 if x < 1 << 7 else 2 if x < 1 << 14 else 3 if x < 1 << 21 else 4 if x < 1 << 28 else 5


def lcp_of(a: bytes, b: bytes) -> int:
    n = min(len(a), len(b))
    i = 0
    while i < n and a[i] == b[i]:
        i += 1
    return i


class BlockGen:
    """block_builder.c:52-158."""

    def __init__(self, restart_interval: int):
        self.R = restart_interval
        self.reset()

    def reset(self):
        self.buf = bytearray()
        self.restarts = [0]
        self.counter = 0
        self.last = b""

    def empty(self) -> bool:
        return not self.buf

    def add(self, key: bytes, value: bytes):
        shared = 0
        if self.counter < self.R:
            shared = lcp_of(self.last, key)
        else:
            self.restarts.append(len(self.buf))
            self.counter = 0
        self.buf += varint(shared) + varint(len(key) - shared) + varint(len(value))
        self.buf += key[shared:] + value
        self.last = key
        self.counter += 1

    def estimate(self) -> int:
        return len(self.buf) + 4 * len(self.restarts) + 4

    def finish(self) -> bytes:
        return bytes(self.buf) + b"".join(struct.pack("<I", r) for r in self.restarts) + \
            struct.pack("<I", len(self.restarts))


def serial_blocks(entries, block_size: int, restart_interval: int = 16):
    """(block_first with nblocks+1 values, raw data blocks): the serial rule."""
    gen = BlockGen(restart_interval)
    first, blocks = [0], []
    for i, (k, v) in enumerate(entries):
        gen.add(k, v)
        if gen.estimate() >= block_size:
            blocks.append(gen.finish())
            gen.reset()
            first.append(i + 1)
    if not gen.empty():
        blocks.append(gen.finish())
        first.append(len(entries))
    return first, blocks


def _bytewise_separator(start: bytes, limit: bytes) -> bytes:   # comparator.c:44-70
    d = lcp_of(start, limit)
    if d < min(len(start), len(limit)) and start[d] < 0xff and start[d] + 1 < limit[d]:
        return start[:d] + bytes([start[d] + 1])
    return start


def _bytewise_successor(key: bytes) -> bytes:                   # comparator.c:72-88
    for i, c in enumerate(key):
        if c != 0xff:
            return key[:i] + bytes([c + 1])
    return key


def separator(start: bytes, limit: bytes, internal: bool) -> bytes:
    if not internal:
        return _bytewise_separator(start, limit)
    us, ul = start[:-8], limit[:-8]                             # dbformat.c:232-260
    t = _bytewise_separator(us, ul)
    return t + MAX_SEQ_SEEK if len(t) < len(us) and us < t else start


def successor(key: bytes, internal: bool) -> bytes:
    if not internal:
        return _bytewise_successor(key)
    uk = key[:-8]                                               # dbformat.c:262-285
    t = _bytewise_successor(uk)
    return t + MAX_SEQ_SEEK if len(t) < len(uk) and uk < t else key


def index_keys(entries, first, internal: bool):
    nb = len(first) - 1
    out = []
    for b in range(nb):
        last = entries[first[b + 1] - 1][0]
        out.append(separator(last, entries[first[b + 1]][0], internal) if b + 1 < nb
                   else successor(last, internal))
    return out


def parallel_first(entries, block_size: int, restart_interval: int = 16):
    """block_first by steps 1-4 of the parallel formulation."""
    import numpy as np
    n, R = len(entries), restart_interval
    if n == 0:
        return [0]
    sh = np.zeros(n, dtype=np.int64)
    d = np.zeros(n, dtype=np.int64)
    for i, (k, v) in enumerate(entries):
        l = lcp_of(entries[i - 1][0], k) if i else 0
        sh[i] = vl(l) + vl(len(k) - l) + vl(len(v)) + len(k) - l + len(v)
        d[i] = 1 + vl(len(k)) + vl(len(v)) + len(k) + len(v) - sh[i]
    S = np.concatenate([[0], np.cumsum(sh)])
    C = d.copy()                                   # Hillis-Steele over stride R
    step = R
    while step < n:
        C[step:] = C[step:] + C[:-step].copy()
        step *= 2

    s = np.arange(n, dtype=np.int64)
    c_before = np.where(s >= R, C[np.maximum(s - R, 0)], 0)

    def est(j):                                    # of the block s..j, for every s at once
        m = j - s + 1
        return S[j + 1] - S[s] + C[s + (j - s) // R * R] - c_before + 4 * -(-m // R) + 4

    lo, hi = s.copy(), np.full(n, n, dtype=np.int64)
    while (lo < hi).any():                         # first j with est >= block_size, else n
        mid = np.minimum((lo + hi) // 2, n - 1)
        open_ = lo < hi
        reached = est(mid) >= block_size
        hi = np.where(open_ & reached, mid, hi)
        lo = np.where(open_ & ~reached, mid + 1, lo)
    nxt = np.zeros(n + 1, dtype=np.int64)
    nxt[n] = n
    nxt[:n] = np.minimum(lo + 1, n)
    mark = np.zeros(n + 1, dtype=bool)
    mark[0] = True
    J = nxt
    for _ in range(max(1, n.bit_length())):        # >= ceil(log2(n+1)) rounds
        mark[J[mark]] = True
        J = J[J]
    return [int(i) for i in np.nonzero(mark[:n])[0]] + [n]


def random_entries(rng: random.Random, n: int):
    """Strictly increasing keys with long shared prefixes and varint edges."""
    keys = set()
    alpha = rng.choice([b"ab", b"abc\xff", bytes(range(256))])
    while len(keys) < n:
        ln = rng.choice([1, 2, 5, 16, 16, 24, 130, 200])
        keys.add(bytes(rng.choice(alpha) for _ in range(rng.randrange(1, ln + 1))))
    out = []
    for k in sorted(keys):
        out.append((k, bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 4, 100, 127, 128, 300])))))
    return out


def main() -> None:
    sets = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    rng = random.Random(20240)
    blocks = 0
    for t in range(sets):
        n = rng.choice([0, 1, 2, 15, 16, 17, 33, 100, 700]) if t % 3 else rng.randrange(0, 700)
        e = random_entries(rng, n)
        bs = rng.choice([1, 20, 64, 256, 1024, 4096, 65536])
        R = rng.choice(RESTARTS)
        want, _ = serial_blocks(e, bs, R)
        got = parallel_first(e, bs, R)
        assert got == want, (t, n, bs, R)
        blocks += len(want) - 1
    print(f"{sets} entry sets, {blocks} blocks: the parallel cut equals the serial rule")


if __name__ == "__main__":
    main()
