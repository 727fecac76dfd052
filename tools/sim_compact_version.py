#!/usr/bin/env python3
"""Compaction inside a version: the two pieces of
ldb_do_compaction_work's loop (db_impl.c:1352-1425) that depend on the levels
below the output, ldb_compaction_should_stop_before (version_set.c:2324-2351)
and ldb_compaction_is_base_level_for_key (:2289-2321), serial as lcdb writes
them and in the formulation lgs_merge.hip and lgs_block.hip run.

A level is a list of ``(smallest_ikey, largest_ikey, file_size)`` in the
level's order; ``levels[0]`` is level + 2, the grandparents.

Serial: ``compact_serial`` is the loop over an already merged entry list, with
both functions carrying lcdb's state (grandparent_index, seen_key,
overlapped_bytes, level_ptrs) and sim_table_split's TableGen as the builder.

Parallel:
  1. G(i) = files of level + 2 whose largest key is < key i under the
     internal comparator (the raw tag), a search per entry; pg[i] = P[G(i)],
     P the exclusive prefix sum of the file sizes.  pg does not decrease.
  2. overlapped_bytes before entry i is pg[i] less pg at the last stop, or at
     entry 0 (what the first key passes costs nothing: seen_key).  So the stop
     behind i is the first i' > i with pg[i'] - pg[i] > limit, a search, and
     the stops are what that relation reaches from entry 0 by pointer
     doubling.  Entry 0 is the root, not a stop.
  3. base(user key) is a search per level: the first file whose largest user
     key is >= the key must not exist or must start behind the key.  It stands
     where drop_deletions stands in sim_merge.drop_flags.
  4. a stop closes the output file only when one is open, so kept entry k > 0
     is a forced file start exactly when a stop lies behind the position of
     kept entry k - 1 and not behind its own: the counts of stops up to either
     position differ.
  5. forced cut: next(s) = min(next by size, first forced index > s); forced
     file plan: a file ends after the first block that reaches
     max_output_file_size or before the next block whose first entry is
     forced.  Both are reached from 0 by doubling, as §4.5 and §4.9 have it.

usage: python tools/sim_compact_version.py [CASES]      (seeded random cases)
"""
from __future__ import annotations

import os
import random
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sim_merge  # noqa: E402
import sim_table_split  # noqa: E402
from sim_block_cut import BlockGen  # noqa: E402
from sim_merge import MAX_SEQUENCE, TYPE_DELETION, compare, parsable, tag_of  # noqa: E402

MAX_LEVELS = 5


# ---- serial: lcdb's functions with their state ------------------------------

class Compaction:
    """The fields of ldb_compaction_t the two functions use."""

    def __init__(self, levels, limit: int):
        assert len(levels) <= MAX_LEVELS
        self.levels, self.limit = levels, limit
        self.grandparents = levels[0] if levels else []
        self.grandparent_index = 0
        self.seen_key = False
        self.overlapped_bytes = 0
        self.level_ptrs = [0] * len(levels)

    def should_stop_before(self, ikey: bytes) -> bool:          # version_set.c:2324-2351
        g = self.grandparents
        while self.grandparent_index < len(g) and \
                compare(ikey, g[self.grandparent_index][1], True) > 0:
            if self.seen_key:
                self.overlapped_bytes += g[self.grandparent_index][2]
            self.grandparent_index += 1
        self.seen_key = True
        if self.overlapped_bytes > self.limit:
            self.overlapped_bytes = 0
            return True
        return False

    def is_base_level_for_key(self, ukey: bytes) -> bool:       # :2289-2321
        for lv, files in enumerate(self.levels):
            while self.level_ptrs[lv] < len(files):
                lo, hi, _ = files[self.level_ptrs[lv]]
                if ukey <= hi[:-8]:
                    if ukey >= lo[:-8]:
                        return False
                    break
                self.level_ptrs[lv] += 1
        return True


def loop_serial(keys, smallest_snapshot: int, levels, limit: int):
    """db_impl.c:1352-1397 over the merged keys: (stop flags, drop flags)."""
    c = Compaction(levels, limit)
    stops, drops = [], []
    user_key, has_user_key, last = b"", False, MAX_SEQUENCE
    for k in keys:
        stops.append(c.should_stop_before(k))                    # :1354
        drop = False
        if not parsable(k):                                      # :1363-1367
            user_key, has_user_key, last = b"", False, MAX_SEQUENCE
        else:
            if not has_user_key or k[:-8] != user_key:
                user_key, has_user_key, last = k[:-8], True, MAX_SEQUENCE
            t = tag_of(k)
            if last <= smallest_snapshot:                        # (A)
                drop = True
            elif (t & 0xff) == TYPE_DELETION and (t >> 8) <= smallest_snapshot and \
                    c.is_base_level_for_key(k[:-8]):             # :1379-1382
                drop = True
            last = t >> 8
        drops.append(drop)
    return stops, drops


def compact_serial(entries, smallest_snapshot: int, levels, limit: int, block_size: int = 4096,
                   restart_interval: int = 16, compression: int = 0, bits_per_key: int = 0,
                   max_file_size: int = sim_table_split.NO_SPLIT):
    """db_impl.c:1352-1434 over merged (key, value) entries: (kept entries,
    file_first over the kept entries with files + 1 values, file images)."""
    assert max_file_size >= 1
    c = Compaction(levels, limit)
    kept, first, images, gen = [], [], [], None
    user_key, has_user_key, last = b"", False, MAX_SEQUENCE
    for k, v in entries:
        if c.should_stop_before(k) and gen is not None:          # :1354-1360
            images.append(gen.finish())
            gen = None
        drop = False
        if not parsable(k):
            user_key, has_user_key, last = b"", False, MAX_SEQUENCE
        else:
            if not has_user_key or k[:-8] != user_key:
                user_key, has_user_key, last = k[:-8], True, MAX_SEQUENCE
            t = tag_of(k)
            if last <= smallest_snapshot:
                drop = True
            elif (t & 0xff) == TYPE_DELETION and (t >> 8) <= smallest_snapshot and \
                    c.is_base_level_for_key(k[:-8]):
                drop = True
            last = t >> 8
        if drop:
            continue
        if gen is None:                                          # :1401-1406
            gen = sim_table_split.TableGen(block_size, restart_interval, compression,
                                           bits_per_key, True)
            first.append(len(kept))
        kept.append((k, v))
        gen.add(k, v)                                            # :1415
        if gen.size() >= max_file_size:                          # :1418-1424
            images.append(gen.finish())
            gen = None
    if gen is not None:                                          # :1433-1434
        images.append(gen.finish())
    return kept, first + [len(kept)], images


# ---- parallel ---------------------------------------------------------------

def passed(keys, grandparents):
    """G(i) per key, by bisection over the files' largest keys."""
    out = []
    for k in keys:
        lo, hi = 0, len(grandparents)
        while lo < hi:
            mid = (lo + hi) // 2
            if compare(grandparents[mid][1], k, True) >= 0:
                hi = mid
            else:
                lo = mid + 1
        out.append(lo)
    return out


def reach(nxt, n: int):
    """What nxt reaches from 0 by pointer doubling: marks, n of them."""
    mark = [False] * (n + 1)
    if n:
        mark[0] = True
    jump = list(nxt) + [n]
    for _ in range(max(1, n.bit_length())):
        for s in range(n):
            if mark[s]:
                mark[jump[s]] = True
        jump = [jump[j] for j in jump]
    return mark[:n]


def stops_chain(keys, levels, limit: int):
    """Steps 1 and 2: the stop flags."""
    n = len(keys)
    g = levels[0] if levels else []
    P = [0]
    for f in g:
        P.append(P[-1] + f[2])
    pg = [P[x] for x in passed(keys, g)]
    nxt = []
    for i in range(n):
        lo, hi = i + 1, n
        while lo < hi:
            mid = (lo + hi) // 2
            if pg[mid] - pg[i] > limit:
                hi = mid
            else:
                lo = mid + 1
        nxt.append(lo)
    mark = reach(nxt, n)
    if n:
        mark[0] = False
    return mark


def base_search(levels, ukey: bytes) -> bool:
    """Step 3."""
    for files in levels:
        lo, hi = 0, len(files)
        while lo < hi:
            mid = (lo + hi) // 2
            if files[mid][1][:-8] >= ukey:
                hi = mid
            else:
                lo = mid + 1
        if lo < len(files) and files[lo][0][:-8] <= ukey:
            return False
    return True


def drop_flags(keys, smallest_snapshot: int, levels):
    """sim_merge.drop_flags with base_search per entry for drop_deletions."""
    out = []
    for i, k in enumerate(keys):
        last = MAX_SEQUENCE
        if i and keys[i - 1][:-8] == k[:-8] and parsable(keys[i - 1]):
            last = tag_of(keys[i - 1]) >> 8
        t = tag_of(k)
        out.append(parsable(k) and
                   (last <= smallest_snapshot or
                    ((t & 0xff) == TYPE_DELETION and (t >> 8) <= smallest_snapshot and
                     base_search(levels, k[:-8]))))
    return out


def forced_flags(stops, drops):
    """Step 4: one flag per kept entry."""
    cnt, acc = [], 0
    for s, d in zip(stops, drops):
        acc += bool(s)
        if not d:
            cnt.append(acc)
    return [k > 0 and cnt[k] != cnt[k - 1] for k in range(len(cnt))]


def first_forced(flags, s: int, e: int) -> int:
    """The first index in (s, e) whose flag is set, else e: a search over the
    flags' prefix sums."""
    F = [0]
    for f in flags:
        F.append(F[-1] + bool(f))
    if F[e] == F[s + 1]:
        return e
    lo, hi = s + 1, e - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if F[mid + 1] > F[s + 1]:
            hi = mid
        else:
            lo = mid + 1
    return lo


def forced_cut(entries, forced, block_size: int, restart_interval: int):
    """Step 5, blocks: block_first with blocks + 1 values."""
    n = len(entries)
    nxt = []
    for s in range(n):
        gen = BlockGen(restart_interval)                         # next by size: the serial
        e = n                                                    # estimate from s (§4.5 has
        for j in range(s, n):                                    # it as a search)
            gen.add(*entries[j])
            if gen.estimate() >= block_size:
                e = j + 1
                break
        nxt.append(first_forced(forced, s, e))
    mark = reach(nxt, n)
    return [i for i in range(n) if mark[i]] + [n]


def block_bytes(entries, bfirst, restart_interval: int):
    out = []
    for b in range(len(bfirst) - 1):
        gen = BlockGen(restart_interval)
        for k, v in entries[bfirst[b]:bfirst[b + 1]]:
            gen.add(k, v)
        out.append(gen.finish())
    return out


def forced_files(entries, forced, bfirst, block_size: int, restart_interval: int, compression: int,
                 max_file_size: int):
    """Step 5, files: file_first with files + 1 values."""
    import oracle
    nb = len(bfirst) - 1
    if nb == 0:
        return [0]
    _, hoff, hsize, _ = oracle.table_write_blocks(block_bytes(entries, bfirst, restart_interval),
                                                  compression, 0)
    start = [int(x) for x in hoff]
    end = [int(o) + int(s) + 5 for o, s in zip(hoff, hsize)]
    fflag = [bool(forced[bfirst[b]]) for b in range(nb)]
    nxt = []
    for s in range(nb):
        lo, hi = s, nb
        while lo < hi:
            mid = (lo + hi) // 2
            if end[mid] - start[s] >= max_file_size:
                hi = mid
            else:
                lo = mid + 1
        nxt.append(first_forced(fflag, s, min(lo + 1, nb)))
    mark = reach(nxt, nb)
    return [bfirst[b] for b in range(nb) if mark[b]] + [len(entries)]


def file_images(entries, file_first, block_size: int, restart_interval: int, compression: int,
                bits_per_key: int):
    """Per file the builder's image (§4.9's per-file work is unchanged)."""
    out = []
    for f in range(len(file_first) - 1):
        gen = sim_table_split.TableGen(block_size, restart_interval, compression, bits_per_key, True)
        for k, v in entries[file_first[f]:file_first[f + 1]]:
            gen.add(k, v)
        out.append(gen.finish())
    return out


def compact_parallel(entries, smallest_snapshot: int, levels, limit: int, block_size: int = 4096,
                     restart_interval: int = 16, compression: int = 0, bits_per_key: int = 0,
                     max_file_size: int = sim_table_split.NO_SPLIT):
    """compact_serial's results by steps 1-5."""
    keys = [k for k, _ in entries]
    stops = stops_chain(keys, levels, limit)
    drops = drop_flags(keys, smallest_snapshot, levels)
    kept = [e for e, d in zip(entries, drops) if not d]
    forced = forced_flags(stops, drops)
    bfirst = forced_cut(kept, forced, block_size, restart_interval)
    first = forced_files(kept, forced, bfirst, block_size, restart_interval, compression,
                         max_file_size)
    return kept, first, file_images(kept, first, block_size, restart_interval, compression,
                                    bits_per_key)


# ---- random cases -------------------------------------------------------------

def ikey(user: bytes, seq: int, typ: int) -> bytes:
    return user + struct.pack("<Q", (seq << 8) | typ)


def random_levels(rng: random.Random, nlevels: int, users):
    """Disjoint files over the sorted user keys `users`, with gaps."""
    levels = []
    for _ in range(nlevels):
        files, i = [], rng.randrange(0, 3)
        while i < len(users) and rng.random() < 0.9:
            j = min(len(users) - 1, i + rng.randrange(0, 4))
            lo = ikey(users[i], rng.randrange(1, 40), 1)
            hi = ikey(users[j], rng.randrange(0, 40) if j > i else 0, rng.randrange(0, 2))
            if compare(lo, hi, True) > 0:
                lo, hi = hi, lo
            files.append((lo, hi, rng.choice([0, 1, 10, 100, 1000])))
            i = j + rng.randrange(1, 4)
        levels.append(files)
    return levels


def random_case(rng: random.Random):
    nu = rng.choice([1, 2, 5, 20, 60])
    users = sorted({bytes(rng.choice(b"ab\0\xff") for _ in range(rng.randrange(0, 6)))
                    for _ in range(nu)})
    entries = []
    for u in users:
        for s in sorted(rng.sample(range(1, 60), rng.choice([1, 1, 2, 3])), reverse=True):
            typ = rng.choice([0, 0, 1, 1, 1, 2]) if rng.random() < 0.1 else rng.choice([0, 1, 1])
            entries.append((ikey(u, s, typ), bytes(rng.randrange(256)
                                                   for _ in range(rng.choice([0, 3, 40])))))
    entries.sort(key=sim_merge.sort_key(True))
    more = sorted(set(users) | {u + b"\0" for u in users[:3]} | {b"", b"\xff\xff\xff\xff\xff\xff\xff"})
    levels = random_levels(rng, rng.randrange(0, MAX_LEVELS + 1), more)
    return (entries, rng.choice([0, 10, 30, 59, 100]), levels,
            rng.choice([0, 1, 10, 99, 100, 101, 1000, 5000]))


def main() -> None:
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rng = random.Random(20251)
    files = 0
    for t in range(cases):
        entries, snap, levels, limit = random_case(rng)
        keys = [k for k, _ in entries]
        stops, drops = loop_serial(keys, snap, levels, limit)
        assert stops_chain(keys, levels, limit) == stops, t
        assert drop_flags(keys, snap, levels) == drops, t
        args = (rng.choice([1, 64, 256]), rng.choice([1, 3, 16]), rng.choice([0, 1]),
                rng.choice([0, 10]), rng.choice([1, 100, 400, sim_table_split.NO_SPLIT]))
        want = compact_serial(entries, snap, levels, limit, *args)
        assert compact_parallel(entries, snap, levels, limit, *args) == want, t
        files += len(want[2])
    print(f"{cases} cases, {files} files: the parallel formulation equals lcdb's loop")


if __name__ == "__main__":
    main()
