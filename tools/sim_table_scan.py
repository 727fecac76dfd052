#!/usr/bin/env python3
"""lcdb's forward table scan over bytes, in plain Python.

The reference restated: ldb_blockiter_first + ldb_blockiter_next until invalid
(block.c:247-296, 411-415) as `block_walk`; ldb_tableiter_create, then first
or seek, then next until invalid (two_level_iterator.c over table.c:229-300)
as `scan`.  Beside them the formulations lgs_scan.hip and lgs_table_scan use,
each an independent restatement that the tests hold against the first:

* `block_walk_links`: the header walk writes per entry where its key delta
  lies, its `shared` count and a link to the nearest earlier entry with a
  smaller `shared`; a key is then rebuilt from the block's bytes alone by
  following links, every step lowering the prefix still needed;
* `index_entries`: the index block parsed a restart slot at a time, which is
  the serial walk whenever every slot's entry has shared = 0 and ends where
  the next slot's begins, with the serial walk as the fallback;
* `scan_window` / `scan_windows`: the scan a window of index entries at a
  time, a seek's window begun in the restart run the data seek chose.

Statuses are the LGS_ST_* codes; tests/golden/table_scan.bin pins this file.

usage: python tools/sim_table_scan.py TABLE.ldb [START]   (bytewise keys)
"""
from __future__ import annotations

import bisect
import hashlib
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sim_table_get import (ST_CORRUPT, ST_OK, Table, block_seek, block_seek_prefix,  # noqa: E402
                           compare, decode_entry, handle_import, read_block)

NONE = 0xFFFFFFFF


def _open(block: bytes):
    """ldb_blockiter_create's checks: (status, restart array offset or None)."""
    size = len(block)
    if size < 4:
        return ST_CORRUPT, None
    nr = struct.unpack_from("<I", block, size - 4)[0]
    if nr > (size - 4) // 4:
        return ST_CORRUPT, None
    if nr == 0:
        return ST_OK, None
    return ST_OK, size - (1 + nr) * 4


def _headers(block: bytes, internal: bool, walk_from, first_unchecked: bool = False):
    """The header walk: (status, [(entry offset, shared, non_shared, value
    length, key delta offset)]) from walk_from (None: restart[0]) on."""
    st, restarts = _open(block)
    if restarts is None:
        return st, []
    cur = struct.unpack_from("<I", block, restarts)[0] if walk_from in (None, NONE) else walk_from
    cur = min(cur, restarts)
    out, klen = [], (1 << 40 if first_unchecked else 0)
    while cur < restarts:
        e = decode_entry(block, cur, restarts)
        if e is None or klen < e[0] or (internal and e[0] + e[1] < 8):
            return ST_CORRUPT, out
        out.append((cur,) + e)
        klen = e[0] + e[1]
        cur = e[3] + e[1] + e[2]
    return ST_OK, out


def block_walk(block: bytes, internal: bool = False, walk_from=None, emit_from=None):
    """(status, [(entry offset, key, value)]): the iterator's walk, its key
    buffer cut back to `shared` and extended at every entry (block.c:278-281).
    Entries before offset emit_from are parsed but not delivered."""
    st, heads = _headers(block, internal, walk_from)
    key, out = b"", []
    for pos, shared, non_shared, vlen, p in heads:
        key = key[:shared] + block[p:p + non_shared]
        if emit_from in (None, NONE) or pos >= emit_from:
            out.append((pos, key, block[p + non_shared:p + non_shared + vlen]))
    return st, out


def links(shared):
    """link[i]: the nearest j < i with shared[j] < shared[i] (None when
    shared[i] = 0), by following the links already made.  A link that one
    entry steps over is never looked at by a later one, so the whole pass is
    linear in the entries."""
    link, steps = [], 0
    for i, s in enumerate(shared):
        j = None
        if s:
            j = i - 1
            while shared[j] >= s:
                j = link[j]
                steps += 1
        link.append(j)
    assert steps <= 2 * len(shared)
    return link


def block_walk_links(block: bytes, internal: bool = False, walk_from=None, emit_from=None):
    """block_walk as lgs_scan.hip runs it: every key from the block's bytes,
    never from another entry's key.  Bytes [shared, length) are the entry's own
    delta; bytes [0, shared) come from earlier entries: entry j = link[i]
    supplies [shared_j, need), then need = shared_j and j = link[j], until
    need = 0.  Each step lowers `need`, so a key costs at most its length in
    steps whatever the block holds."""
    st, heads = _headers(block, internal, walk_from)
    shared = [h[1] for h in heads]
    link = links(shared)
    out = []
    for i, (pos, sh, non_shared, vlen, p) in enumerate(heads):
        if emit_from not in (None, NONE) and pos < emit_from:
            continue
        key = bytearray(sh + non_shared)
        key[sh:] = block[p:p + non_shared]
        need, j, steps = sh, i, 0
        while need:
            j = link[j]
            sj, pj = heads[j][1], heads[j][4]
            assert sj < need and need - sj <= heads[j][2]
            key[sj:need] = block[pj:pj + need - sj]
            need = sj
            steps += 1
        assert steps <= len(key)
        out.append((pos, bytes(key), block[p + non_shared:p + non_shared + vlen]))
    return st, out


# ---- the index entry list ---------------------------------------------------

def index_walk_serial(index: bytes, internal: bool, walk_from=None):
    """(status, [(entry offset, handle or None)]) by the serial walk; from an
    entry a seek has found, its `shared` is not checked again."""
    st, heads = _headers(index, internal, walk_from, first_unchecked=walk_from is not None)
    return st, [(pos, handle_import(index[p + ns:p + ns + vl])) for pos, _, ns, vl, p in heads]


def index_slots(index: bytes, internal: bool):
    """The speculative parse, a lane per restart slot: (status, entries) when
    every slot agrees, None when one does not."""
    st, restarts = _open(index)
    if restarts is None:
        return st, []
    nr = (len(index) - restarts) // 4 - 1
    slot = [struct.unpack_from("<I", index, restarts + 4 * k)[0] for k in range(nr)]
    if nr == 1 and slot[0] >= restarts:
        return ST_OK, []                      # the empty table's index block
    out = []
    for k in range(nr):
        at, end = slot[k], (slot[k + 1] if k + 1 < nr else restarts)
        if not (at < restarts and end <= restarts and at < end):
            return None
        e = decode_entry(index, at, restarts)
        if e is None or e[0] != 0 or (internal and e[1] < 8) or e[3] + e[1] + e[2] != end:
            return None
        out.append((at, handle_import(index[e[3] + e[1]:e[3] + e[1] + e[2]])))
    return ST_OK, out


def index_entries(index: bytes, internal: bool):
    """(status, entries, fell back): the slots when they agree, else the walk."""
    r = index_slots(index, internal)
    if r is not None:
        return r[0], r[1], False
    st, ents = index_walk_serial(index, internal)
    return st, ents, True


# ---- the table scan ---------------------------------------------------------

def _read(t: Table, h, verify: bool):
    """table.c:229-300 for one index value: (status, contents)."""
    if h is None:
        return ST_CORRUPT, None                                       # table.c:244-245
    return read_block(t.file, h[0], h[1], verify)


def scan(t: Table, verify: bool = True, start: bytes | None = None):
    """ldb_tableiter_create, first (or seek(start)), next until invalid:
    (final status, [(key, value)]).  A table that did not open has no
    iterator: its status and nothing."""
    if t.index is None:
        return t.status, []
    out, saved = [], ST_OK

    def save(st):
        nonlocal saved
        if saved == ST_OK and st != ST_OK:                            # ldb_twoiter_saverr
            saved = st

    first = True
    if start is None:
        ist, ents = index_walk_serial(t.index, t.internal)
    else:
        ist, e = block_seek(t.index, start, t.internal)
        if e is None:
            return ist, []
        ist, ents = index_walk_serial(t.index, t.internal, walk_from=e[0])
    for _, h in ents:
        st, block = _read(t, h, verify)
        if st != ST_OK:
            save(st)
        elif start is not None and first:
            # ldb_twoiter_seek: a fresh data iterator seeks; next goes on from
            # the restart run that seek chose.
            sst, f = block_seek_prefix(block, start, t.internal)
            if f is None:
                save(sst)
            else:
                bst, es = block_walk(block, t.internal, walk_from=f[4], emit_from=f[0])
                out += [(k, v) for _, k, v in es]
                save(bst)
        else:
            bst, es = block_walk(block, t.internal)
            out += [(k, v) for _, k, v in es]
            save(bst)
        first = False
    return (ist if ist != ST_OK else saved), out


class IndexList:
    """What an opened table keeps after its first scan."""

    def __init__(self, t: Table):
        self.status, self.entries, self.fell_back = (
            (t.status, [], False) if t.index is None else index_entries(t.index, t.internal))
        self.pos = [p for p, _ in self.entries]


def scan_window(t: Table, lst: IndexList, verify: bool = True, start: bytes | None = None,
                first_block: int = 0, max_blocks: int = 1 << 30):
    """One call of lgs_table_scan: a dict of entries [(key, value)],
    block_entry_first, block_status, blocks_done, next_block, at_end,
    index_status; or {"need_blocks": k} where the C call returns LGS_ENOSPC
    for its window's length."""
    res = {"entries": [], "block_entry_first": [0], "block_status": [], "blocks_done": 0,
           "next_block": first_block, "at_end": True, "index_status": lst.status}
    if t.index is None:
        return res
    seek = start is not None
    if seek:
        ist, e = block_seek(t.index, start, t.internal)
        if e is None:
            res["index_status"], res["next_block"] = ist, len(lst.entries)
            return res
        m = bisect.bisect_left(lst.pos, e[0])
        if m < len(lst.pos) and lst.pos[m] == e[0]:
            b0, window = m, None
        else:
            # Off the forward walk's path: up to where the two walks meet.
            sst, side = index_walk_serial(t.index, t.internal, walk_from=e[0])
            k, join = len(side), None
            for i, (p, _) in enumerate(side):
                j = bisect.bisect_left(lst.pos, p)
                if j < len(lst.pos) and lst.pos[j] == p:
                    k, join = i, j
                    break
            if k > max_blocks:
                return {"need_blocks": k}
            window = side[:k]
            res["next_block"] = len(lst.entries) if join is None else join
            res["at_end"] = join is None
            if join is None:
                res["index_status"] = sst
    else:
        b0, window = first_block, None
    if window is None:
        b0 = min(b0, len(lst.entries))
        window = lst.entries[b0:b0 + max_blocks]
        res["next_block"] = b0 + len(window)
        res["at_end"] = res["next_block"] >= len(lst.entries)
    res["blocks_done"] = len(window)
    for j, (_, h) in enumerate(window):
        st, block = _read(t, h, verify)
        if st == ST_OK and seek and j == 0:
            st, f = block_seek_prefix(block, start, t.internal)
            es = []
            if f is not None:
                st, es = block_walk_links(block, t.internal, walk_from=f[4], emit_from=f[0])
        elif st == ST_OK:
            st, es = block_walk_links(block, t.internal)
        else:
            es = []
        res["entries"] += [(k, v) for _, k, v in es]
        res["block_entry_first"].append(len(res["entries"]))
        res["block_status"].append(st)
    return res


def scan_windows(t: Table, verify: bool = True, start: bytes | None = None, max_blocks: int = 64,
                 end: bytes | None = None):
    """OpenTable.scan's loop: (final status, [(key, value)]), cut at the first
    key with compare(key, end) >= 0."""
    lst = IndexList(t)
    out, saved, nxt, first = [], ST_OK, 0, True
    while True:
        r = scan_window(t, lst, verify, start if first else None, nxt, max_blocks)
        if "need_blocks" in r:
            max_blocks = r["need_blocks"]
            continue
        first = False
        ef = r["block_entry_first"]
        for j, st in enumerate(r["block_status"]):
            for k, v in r["entries"][ef[j]:ef[j + 1]]:
                if end is not None and compare(k, end, t.internal) >= 0:
                    return saved, out            # the caller's loop leaves a valid iterator
                out.append((k, v))
            if saved == ST_OK and st != ST_OK:
                saved = st
        nxt = r["next_block"]
        if r["at_end"]:
            return (r["index_status"] if r["index_status"] != ST_OK else saved), out


def digest(entries) -> bytes:
    """SHA-256 over the length-prefixed keys and values."""
    h = hashlib.sha256()
    for k, v in entries:
        h.update(struct.pack("<I", len(k)) + k + struct.pack("<I", len(v)) + v)
    return h.digest()


def main() -> None:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t = Table(open(sys.argv[1], "rb").read())
    st, es = scan(t, True, sys.argv[2].encode() if len(sys.argv) > 2 else None)
    for k, v in es:
        print(k, v)
    print("status", st, "entries", len(es))


if __name__ == "__main__":
    main()
