#!/usr/bin/env python3
"""lcdb's block seek and table Get over bytes, in plain Python.

The reference restated: ldb_blockiter_create + ldb_blockiter_seek
(block.c:324-451, decode_entry :86-125, parse_next_key :247-289) as
`block_seek`, ldb_table_open + ldb_table_internal_get (table.c:78-190,
314-364) as `Table.get`, and what version_set.c's save_value (:373-388) makes
of a result as `verdict`.  The seek here rebuilds every key as the reference's
iterator does; lgs_seek.hip carries the prefix it shares with the target
instead, so the two are independent restatements.  Blocks are read through the
oracle's ldb_read_block and bloom restatements (oracle/), which their own
tests pin to the reference; tests/golden/table_get.bin pins this file.

Statuses are the LGS_ST_* codes of include/lcdb_gpu_snappy.h.

usage: python tools/sim_table_get.py TABLE.ldb KEY...   (bytewise keys)
"""
from __future__ import annotations

import struct
import sys

ST_CORRUPT, ST_OK, ST_NOSPACE, ST_IOERR, ST_BADCRC, ST_BADTYPE = 0, 1, 2, 3, 4, 5
NOTFOUND, FOUND, DELETED, CORRUPT = 0, 1, 2, 3
MAGIC = 0xdb4775248b80fb57
FILTER_NAME = b"filter.leveldb.BuiltinBloomFilter2"


def varint(b: bytes, at: int, limit: int, bits: int):
    """coding.h varint32/64 read: (value, next) or None."""
    v, sh = 0, 0
    while at < limit and sh <= (28 if bits == 32 else 63):
        c = b[at]
        at += 1
        v |= (c & 0x7F) << sh
        if c < 0x80:
            return v & ((1 << bits) - 1), at
        sh += 7
    return None


def decode_entry(b: bytes, at: int, limit: int):
    """block.c:86-125: (shared, non_shared, value_length, key delta offset) or None."""
    if limit < at or limit - at < 3:
        return None
    s, n, v = b[at], b[at + 1], b[at + 2]
    if (s | n | v) < 128:
        p = at + 3
    else:
        p = at
        out = []
        for _ in range(3):
            r = varint(b, p, limit, 32)
            if r is None:
                return None
            out.append(r[0])
            p = r[1]
        s, n, v = out
    if limit - p < n + v:
        return None
    return s, n, v, p


def compare(a: bytes, b: bytes, internal: bool) -> int:
    """comparator.c:44-52, or ldb_ikc_compare (dbformat.c:206-230)."""
    if internal:
        ua, ub = a[:-8], b[:-8]
        if ua != ub:
            return -1 if ua < ub else 1
        ta, tb = struct.unpack("<Q", a[-8:])[0], struct.unpack("<Q", b[-8:])[0]
        return -1 if ta > tb else (1 if ta < tb else 0)
    return -1 if a < b else (1 if a > b else 0)


def block_seek(block: bytes, target: bytes, internal: bool = False):
    """(status, None) or (ST_OK, (entry offset, key, value offset, value length))."""
    size = len(block)
    if size < 4:
        return ST_CORRUPT, None
    nr = struct.unpack_from("<I", block, size - 4)[0]
    if nr > (size - 4) // 4:
        return ST_CORRUPT, None
    if nr == 0:
        return ST_OK, None
    restarts = size - (1 + nr) * 4
    if internal and len(target) < 8:
        return ST_CORRUPT, None

    def restart_point(i):
        return min(struct.unpack_from("<I", block, restarts + 4 * i)[0], restarts)

    left, right = 0, nr - 1
    while left < right:
        mid = (left + right + 1) // 2
        e = decode_entry(block, restart_point(mid), restarts)
        if e is None or e[0] != 0 or (internal and e[1] < 8):
            return ST_CORRUPT, None
        if compare(block[e[3]:e[3] + e[1]], target, internal) < 0:
            left = mid
        else:
            right = mid - 1
    cur, key = restart_point(left), b""
    while True:
        if cur >= restarts:
            return ST_OK, None
        e = decode_entry(block, cur, restarts)
        if e is None or len(key) < e[0] or (internal and e[0] + e[1] < 8):
            return ST_CORRUPT, None
        shared, non_shared, vlen, p = e
        key = key[:shared] + block[p:p + non_shared]
        if compare(key, target, internal) >= 0:
            return ST_OK, (cur, key, p + non_shared, vlen)
        cur = p + non_shared + vlen


def _lcp(a: bytes, ai: int, b: bytes, bi: int, n: int) -> int:
    i = 0
    while i < n and a[ai + i] == b[bi + i]:
        i += 1
    return i


def _key_bytes(block: bytes, start: int, entry: int, limit: int, pos: int) -> bytes:
    """Bytes [pos, pos + 8) of the key of the entry at `entry`, by walking its
    restart run again: each entry puts its delta at [shared, shared + non_shared)."""
    r = bytearray(8)
    at = start
    while at <= entry:
        shared, non_shared, vlen, p = decode_entry(block, at, limit)
        for j in range(8):
            x = pos + j
            if shared <= x < shared + non_shared:
                r[j] = block[p + x - shared]
        at = p + non_shared + vlen
    return bytes(r)


def block_seek_prefix(block: bytes, target: bytes, internal: bool = False):
    """block_seek as lgs_seek.hip runs it: the scan does not rebuild the key.
    It carries `pre`, the length of the prefix the current key shares with
    the target's user key (at most either's length), and `kb`, the key's byte
    behind that prefix; an entry whose `shared` reaches past `pre` keeps both.
    Same result as block_seek, the found key left out:
    (status, None) or (ST_OK, (entry offset, key length, value offset, value
    length, start of the restart run))."""
    size = len(block)
    if size < 4:
        return ST_CORRUPT, None
    nr = struct.unpack_from("<I", block, size - 4)[0]
    if nr > (size - 4) // 4:
        return ST_CORRUPT, None
    if nr == 0:
        return ST_OK, None
    restarts = size - (1 + nr) * 4
    trim = 8 if internal else 0
    tn = len(target)
    if tn < trim:
        return ST_CORRUPT, None
    tu = tn - trim

    def restart_point(i):
        return min(struct.unpack_from("<I", block, restarts + 4 * i)[0], restarts)

    def tags(ktag: bytes) -> int:
        a, b = struct.unpack("<Q", ktag)[0], struct.unpack("<Q", target[tu:])[0]
        return -1 if a > b else (1 if a < b else 0)

    left, right = 0, nr - 1
    while left < right:
        mid = (left + right + 1) // 2
        e = decode_entry(block, restart_point(mid), restarts)
        if e is None or e[0] != 0 or e[1] < trim:
            return ST_CORRUPT, None
        _, kn, _, p = e
        ku = kn - trim
        c = min(ku, tu)
        m = _lcp(block, p, target, 0, c)
        if m < c:
            cmp = -1 if block[p + m] < target[m] else 1
        elif ku != tu:
            cmp = -1 if ku < tu else 1
        else:
            cmp = tags(block[p + ku:p + ku + 8]) if trim else 0
        if cmp < 0:
            left = mid
        else:
            right = mid - 1
    start = restart_point(left)
    cur, klen, pre, kb = start, 0, 0, 0
    while True:
        if cur >= restarts:
            return ST_OK, None
        e = decode_entry(block, cur, restarts)
        if e is None or klen < e[0] or e[0] + e[1] < trim:
            return ST_CORRUPT, None
        shared, non_shared, vlen, p = e
        klen = shared + non_shared
        if shared <= pre:
            m = _lcp(block, p, target, shared, min(non_shared, tu - shared))
            pre = shared + m
            if m < non_shared:
                kb = block[p + m]
        ku = klen - trim
        if pre < min(ku, tu):
            cmp = -1 if kb < target[pre] else 1
        elif ku != tu:
            cmp = -1 if ku < tu else 1
        elif trim:
            cmp = tags(block[p + ku - shared:p + ku - shared + 8] if ku >= shared
                       else _key_bytes(block, start, cur, restarts, ku))
        else:
            cmp = 0
        if cmp >= 0:
            return ST_OK, (cur, klen, p + non_shared, vlen, start)
        cur = p + non_shared + vlen


def handle_import(v: bytes):
    """format.c:66-80: (offset, size) or None."""
    a = varint(v, 0, len(v), 64)
    if a is None:
        return None
    b = varint(v, a[1], len(v), 64)
    return None if b is None else (a[0], b[0])


def verdict(found_key: bytes, target: bytes) -> int:
    """save_value (version_set.c:373-388) on handle_result's key."""
    if len(found_key) < 8 or found_key[-8] > 1:
        return CORRUPT
    if found_key[:-8] == target[:-8]:
        return FOUND if found_key[-8] == 1 else DELETED
    return NOTFOUND


def read_block(file: bytes, off: int, size: int, verify: bool):
    """ldb_read_block (format.c:162-270) through the oracle: (status, contents).
    A block inside the file is handed over on its own (nothing in the read
    depends on where it lies), one outside it with the whole file."""
    import oracle
    if off + size + 5 <= len(file):
        file, off = file[off:off + size + 5], 0
    cap = min(size, len(file))
    if off + size < len(file) and file[off + size] == 1:
        r = varint(file, off, off + size, 32)
        cap = min(r[0], 32 * size + 64) if r else 0
    st, data = oracle.table_read_block(file, off, size, verify, cap)
    return (ST_CORRUPT if st == ST_NOSPACE else st), data


class Table:
    """ldb_table_open (table.c:128-190) on a file image."""

    def __init__(self, file: bytes, paranoid_checks: bool = False, internal: bool = False,
                 filter_name: bytes | None = FILTER_NAME):
        self.file, self.internal = file, internal
        self.index, self.filter, self.status = None, None, ST_OK
        self.blocks = {}                        # (offset, size, verify) -> read_block's result
        if len(file) < 48:
            self.status = ST_CORRUPT
            return
        foot = file[-48:]
        hs, at = [], 0
        for _ in range(4):
            r = varint(foot, at, 48, 64)
            if r is None:
                break
            hs.append(r[0])
            at = r[1]
        if struct.unpack("<Q", foot[40:])[0] != MAGIC or len(hs) != 4:
            self.status = ST_CORRUPT
            return
        st, data = read_block(file, hs[2], hs[3], paranoid_checks)
        if st != ST_OK:
            self.status = st
            return
        self.index = data
        if filter_name is None:
            return
        st, meta = read_block(file, hs[0], hs[1], paranoid_checks)      # table.c:81-126
        if st != ST_OK:
            return
        st, e = block_seek(meta, filter_name, False)
        if e is None or e[1] != filter_name:
            return
        h = handle_import(meta[e[2]:e[2] + e[3]])
        if h is None:
            return
        st, data = read_block(file, h[0], h[1], paranoid_checks)
        if st == ST_OK:
            self.filter = data

    def get(self, key: bytes, verify: bool = False):
        """ldb_table_internal_get: (called, status, key, value)."""
        import oracle
        if self.index is None:
            return False, self.status, b"", b""
        ist, e = block_seek(self.index, key, self.internal)
        if e is None:
            return False, ist, b"", b""
        value = self.index[e[2]:e[2] + e[3]]
        h = handle_import(value)
        if self.filter is not None and h is not None and not oracle.bloom_restatement().filter_matches(
                self.filter, h[0], key, self.internal):
            return False, ST_OK, b"", b""
        if h is None:
            return False, ST_CORRUPT, b"", b""                         # table.c:244-245
        at = (h[0], h[1], verify)
        if at not in self.blocks:
            self.blocks[at] = read_block(self.file, h[0], h[1], verify)
        st, block = self.blocks[at]
        if st != ST_OK:
            return False, st, b"", b""
        bst, e = block_seek(block, key, self.internal)
        if e is None:
            return False, bst, b"", b""
        return True, ST_OK, e[1], block[e[2]:e[2] + e[3]]


NO_BLOCK = 0xFFFFFFFF


def index_lookup(t: Table, key: bytes):
    """ldb_table_internal_get up to the block read, as the device steps have
    it: (state, seek status, entry offset, handle, live).  state 0: the index
    seek found no entry; 1: an entry whose value is a handle; 2: one whose
    value is none.  live: the query goes on to read a block (a handle, and no
    filter or a filter match)."""
    import oracle
    ist, e = block_seek(t.index, key, t.internal)
    if e is None:
        return 0, ist, None, None, False
    h = handle_import(t.index[e[2]:e[2] + e[3]])
    if h is None:
        return 2, ist, e[0], None, False
    live = t.filter is None or oracle.bloom_restatement().filter_matches(
        t.filter, h[0], key, t.internal)
    return 1, ist, e[0], h, live


def number_blocks(t: Table, keys):
    """The distinct blocks of a batch as lgs_table_get numbers them
    (live_mark_kernel, the scan of the marks, qblock_kernel): returns
    (pre, qblock, nb, handles).

    pre[q] is the status of a query that reads no block.  A live query marks
    the index entry it found, in an array as long as the index block: the key
    is the entry's offset, not the (offset, size) it carries, so two entries
    with one handle are two blocks.  The exclusive scan of the marks is each
    marked entry's rank, in file order whatever the order of the queries;
    qblock[q] is its entry's rank or NO_BLOCK, nb the number of marks, and
    handles[b] the handle of block b."""
    nq = len(keys)
    if t.index is None:
        return [t.status] * nq, [NO_BLOCK] * nq, 0, []
    marks = [0] * len(t.index)
    pre, pos, handle_at = [], [], {}
    for k in keys:
        state, ist, at, h, live = index_lookup(t, k)
        pre.append(ist if state == 0 else (ST_CORRUPT if state == 2 else ST_OK))
        pos.append(at if live else None)
        if live:
            marks[at] = 1
            handle_at[at] = h
    rank, acc = [], 0
    for m in marks:
        rank.append(acc)
        acc += m
    qblock = [NO_BLOCK if p is None else rank[p] for p in pos]
    handles = [handle_at[at] for at in sorted(handle_at)]
    return pre, qblock, acc, handles


def main() -> None:
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t = Table(open(sys.argv[1], "rb").read())
    for k in sys.argv[2:]:
        print(k, t.get(k.encode()))


if __name__ == "__main__":
    main()
