#!/usr/bin/env python3
"""Model of lgs_merge_*: lcdb's merging iterator, forward half
(src/table/merger.c), and the drop loop of ldb_do_compaction_work
(src/db_impl.c:1363-1397), on runs of (key, value) entries.

Two routes to the same order:

* ``merge_serial`` restates ldb_mergeiter_first / _next: at every step the
  smallest current key wins, and find_smallest (merger.c:107-128) replaces
  its candidate only on a strict ``<``, so among equal keys the
  lowest-numbered run's entry comes first.
* ``merge_ranks`` is what lgs_merge.hip runs: ceil(log2 k) passes that merge
  adjacent pairs of run groups by rank.  An entry of the left group lands at
  its own position plus the lower bound of its key in the right group, one of
  the right group at its position plus the upper bound in the left one; an
  odd group is carried over.  Compares look at a 64-bit word first (the first
  eight bytes of the comparable key, big-endian, zero padded) and only on a
  tie at the rest: bytes from offset 8, the length, then (internal keys) the
  tag, descending.

``drop_flags`` is db_impl.c:1363-1397 with entry i and entry i - 1 of the
merged order only, as the kernel evaluates it; ``drop_serial`` is the loop as
the reference writes it.  The tests hold each pair equal.  A key whose type
byte is above 1 fails ldb_pkey_import (dbformat.c:86-107): lcdb keeps such an
entry and forgets the current user key, so the entry behind it counts as a
first occurrence.  ldb_put cannot write one, but a compaction reads table
files, and lcdb's repairer accepts tables that hold them.
"""
from __future__ import annotations

import struct
from functools import cmp_to_key

MAX_SEQUENCE = (1 << 56) - 1      # LDB_MAX_SEQUENCE
TYPE_DELETION, TYPE_VALUE = 0, 1
MAX_RUNS = 64


def tag_of(key: bytes) -> int:
    return struct.unpack("<Q", key[-8:])[0]


def compare(a: bytes, b: bytes, internal: bool) -> int:
    """comparator.c:44-60, or dbformat.c:232-285 over internal keys."""
    if not internal:
        return (a > b) - (a < b)
    ua, ub = a[:-8], b[:-8]
    if ua != ub:
        return (ua > ub) - (ua < ub)
    ta, tb = tag_of(a), tag_of(b)
    return (ta < tb) - (ta > tb)          # descending


def key_word(key: bytes, internal: bool) -> int:
    u = key[:-8] if internal else key
    return int.from_bytes(u[:8].ljust(8, b"\0"), "big")


def compare_words(a: bytes, b: bytes, internal: bool) -> int:
    """The kernel's compare: the word, then the rest.  The word alone never
    decides between "ab" and "ab\\0": the length takes part."""
    wa, wb = key_word(a, internal), key_word(b, internal)
    if wa != wb:
        return (wa > wb) - (wa < wb)
    ua, ub = (a[:-8], b[:-8]) if internal else (a, b)
    m = min(len(ua), len(ub))
    ra, rb = ua[8:m], ub[8:m]
    if ra != rb:
        return (ra > rb) - (ra < rb)
    if len(ua) != len(ub):
        return (len(ua) > len(ub)) - (len(ua) < len(ub))
    if internal:
        ta, tb = tag_of(a), tag_of(b)
        return (ta < tb) - (ta > tb)
    return 0


def check_runs(runs, internal: bool):
    """The plan's precondition check: the lowest-numbered run that is not
    non-decreasing or (internal keys) holds a key under 8 bytes, else None."""
    for r, run in enumerate(runs):
        for i, (k, _) in enumerate(run):
            if internal and len(k) < 8:
                return r
            if i and len(run[i - 1][0]) >= (8 if internal else 0) and \
                    compare(run[i - 1][0], k, internal) > 0:
                return r
    return None


def merge_serial(runs, internal: bool = False):
    """[(run, index)] as ldb_mergeiter_first + _next until invalid deliver."""
    at = [0] * len(runs)
    out = []
    while True:
        best = None
        for r, run in enumerate(runs):                      # merger.c:107-128
            if at[r] < len(run) and (best is None or
                                     compare(run[at[r]][0], runs[best][at[best]][0], internal) < 0):
                best = r
        if best is None:
            return out
        out.append((best, at[best]))
        at[best] += 1


def _bound(group, runs, key: bytes, internal: bool, upper: bool) -> int:
    lo, hi = 0, len(group)
    while lo < hi:
        mid = (lo + hi) // 2
        r, i = group[mid]
        c = compare_words(runs[r][i][0], key, internal)
        if c < 0 or (upper and c == 0):
            lo = mid + 1
        else:
            hi = mid
    return lo


def merge_ranks(runs, internal: bool = False):
    """The same order by the kernel's passes."""
    groups = [[(r, i) for i in range(len(run))] for r, run in enumerate(runs)]
    while len(groups) > 1:
        nxt = []
        for g in range(0, len(groups), 2):
            if g + 1 == len(groups):
                nxt.append(groups[g])                       # the odd group
                continue
            left, right = groups[g], groups[g + 1]
            out = [None] * (len(left) + len(right))
            for p, (r, i) in enumerate(left):
                out[p + _bound(right, runs, runs[r][i][0], internal, False)] = (r, i)
            for p, (r, i) in enumerate(right):
                out[p + _bound(left, runs, runs[r][i][0], internal, True)] = (r, i)
            assert None not in out
            nxt.append(out)
        groups = nxt
    return groups[0] if groups else []


def parsable(key: bytes) -> bool:
    """ldb_pkey_import (dbformat.c:86-107) on a key of at least 8 bytes: the
    tag's type byte is a deletion's or a value's."""
    return key[-8] <= TYPE_VALUE


def drop_flags(keys, smallest_snapshot: int, drop_deletions: bool):
    """Per entry of the merged order (internal keys): True = dropped.  Only
    keys[i] and keys[i - 1] are read: an unparsable entry is kept, and the
    entry behind one starts over at MAX_SEQUENCE like a first occurrence."""
    out = []
    for i, k in enumerate(keys):
        last = MAX_SEQUENCE
        if i and keys[i - 1][:-8] == k[:-8] and parsable(keys[i - 1]):
            last = tag_of(keys[i - 1]) >> 8
        t = tag_of(k)
        out.append(parsable(k) and
                   (last <= smallest_snapshot or
                    ((t & 0xff) == TYPE_DELETION and (t >> 8) <= smallest_snapshot and
                     bool(drop_deletions))))
    return out


def drop_serial(keys, smallest_snapshot: int, drop_deletions: bool):
    """db_impl.c:1363-1397 as written: one walk with its variables, the failed
    ldb_pkey_import ("do not hide error keys") included."""
    out = []
    user_key, has_user_key, last = b"", False, MAX_SEQUENCE
    for k in keys:
        if not parsable(k):                                   # :1363-1367
            user_key, has_user_key, last = b"", False, MAX_SEQUENCE
            out.append(False)
            continue
        if not has_user_key or k[:-8] != user_key:
            user_key, has_user_key, last = k[:-8], True, MAX_SEQUENCE
        t = tag_of(k)
        drop = False
        if last <= smallest_snapshot:
            drop = True
        elif (t & 0xff) == TYPE_DELETION and (t >> 8) <= smallest_snapshot and drop_deletions:
            drop = True
        last = t >> 8
        out.append(drop)
    return out


def merge(runs, internal_keys: bool = False, drop: bool = False, smallest_snapshot: int = 0,
          drop_deletions: bool = False):
    """lgs_merge_host: ([(key, value)], [(run, index)], dropped).  Raises
    ValueError where the C call returns LGS_EINVAL."""
    if len(runs) > MAX_RUNS:
        raise ValueError(f"{len(runs)} runs: at most {MAX_RUNS}")
    if drop and not internal_keys:
        raise ValueError("drop needs internal_keys")
    bad = check_runs(runs, internal_keys)
    if bad is not None:
        raise ValueError(f"run {bad} is not sorted or has a short key")
    order = merge_ranks(runs, internal_keys)
    if drop:
        flags = drop_flags([runs[r][i][0] for r, i in order], smallest_snapshot, drop_deletions)
        kept = [o for o, f in zip(order, flags) if not f]
    else:
        kept = order
    return [runs[r][i] for r, i in kept], kept, len(order) - len(kept)


def visible(entries, snapshot: int):
    """{user key: value} a reader at `snapshot` sees in a set of internal-key
    entries: per user key the newest entry with sequence <= snapshot, and a
    deletion hides the key."""
    best = {}
    for k, v in entries:
        t = tag_of(k)
        seq, typ = t >> 8, t & 0xff
        if seq > snapshot:
            continue
        u = k[:-8]
        if u not in best or best[u][0] < seq:
            best[u] = (seq, typ, v)
    return {u: v for u, (_, typ, v) in best.items() if typ == TYPE_VALUE}


def sort_key(internal: bool):
    return cmp_to_key(lambda a, b: compare(a[0], b[0], internal))


def main() -> None:
    import random
    rng = random.Random(1)
    for _ in range(200):
        internal = rng.random() < 0.5
        k = rng.randrange(0, 9)
        runs = []
        for _r in range(k):
            n = rng.choice([0, 1, 2, 5, 17])
            es = []
            for _i in range(n):
                u = bytes(rng.choice(b"ab\0") for _ in range(rng.randrange(0, 11)))
                key = u + struct.pack("<Q", (rng.randrange(1, 6) << 8) | rng.randrange(2)) \
                    if internal else u
                es.append((key, b"v"))
            runs.append(sorted(es, key=sort_key(internal)))
        assert merge_ranks(runs, internal) == merge_serial(runs, internal)
    print("merge_ranks == merge_serial on 200 random inputs")


if __name__ == "__main__":
    main()
