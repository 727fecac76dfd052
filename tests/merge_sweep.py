"""The generated sweep of the compaction drop: the case list and
the seeded generator of every input entry set, shared by the recipe
(tests/golden/make_merge_sweep_golden.py), the CPU test
(test_merge_sweep_sim.py) and the GPU test (test_gpu_merge_sweep.py).  The
fixture (tests/golden/merge_sweep.bin) stores no inputs.

Two kinds of cases.

``repair``: tables written by lcdb's builder are put at level 0 by
ldb_repair; the DB is opened, the case's script runs (``("s",)`` snapshot,
``("p", key, value)``, ``("d", key)``, ``("f",)`` memtable flush), and
ldb_test_compact_range runs at level 0 and at level 1.  After a repair the
last sequence is the largest *parsable* sequence S in the tables
(repair.c:541-557), a snapshot taken after the open holds S, and the script's
writes take S + 1, S + 2, ...  Entries whose type byte is above 1 (ldb_put
cannot write them; ldb_pkey_import refuses them) may carry any sequence.  The
repairer takes a table's range from its parsable entries only, so every table
begins and ends with a parsable entry.  Level 0 never holds more than three
files (LDB_L0_COMPACTION_TRIGGER is 4).

``wide``: k tables for lcdb's merging iterator alone (the driver's ``merge``
mode); the drop rule over that order is the model's (tools/sim_merge.py), at
each of the case's snapshots and both drop_deletions values.

The sources of a repair case are named: ``t<i>`` the repaired tables, ``f<i>``
the files the script's flushes write, ``o0`` the output of the first step.
"""
from __future__ import annotations

import functools
import os
import random
import sys
from dataclasses import dataclass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sim_merge  # noqa: E402
from merge_helpers import binary_users, ikey  # noqa: E402

MAX_SEQUENCE = sim_merge.MAX_SEQUENCE
S_EDGES = ((1 << 8) - 1, 1 << 24, (1 << 32) - 1, 1 << 32, (1 << 40) + 1, (1 << 56) - 4)
OPTIONS = (4096, 16, 0, 0)          # block_size, restart_interval, compression, bits_per_key
LONG_CHAIN = 300                    # versions of one user key: more than a 256-lane workgroup


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                       # "repair" or "wide"
    family: str
    args: tuple
    ops: tuple = ()                 # repair: the script after the open
    levels: tuple = ()              # repair: files at levels 0-3 before, between, after the steps
    snapshots: tuple = ()           # wide: the smallest_snapshot values


def isorted(es):
    return sorted(es, key=sim_merge.sort_key(True))


def max_parsable(tables) -> int:
    return max(sim_merge.tag_of(k) >> 8 for t in tables for k, _ in t if sim_merge.parsable(k))


# ---- version chains ------------------------------------------------------------

# (offset from S, type byte) per version, newest first; "tie": the one version
# goes to two tables with different values.
PATTERNS = [
    [(2, 2), (0, 1), (-1, 1)],                          # unparsable newest, over S
    [(0, 1), (-1, 0x7f), (-2, 1), (-3, 1)],             # unparsable in the middle, under S
    [(-1, 1), (-2, 1), (-3, 0xff)],                     # unparsable oldest
    [(-1, 1), (-2, 2), (-3, 0xff), (-4, 1), (-5, 1)],   # two in a row
    [(0, 0x7f), (-1, 1), (-2, 1)],                      # unparsable at S itself
    [(1, 0xff), (0, 0), (-1, 1)],                       # a deletion at S directly behind one
    [(-1, 1), (-2, 2), (-3, 0), (-4, 1)],               # a deletion under S directly behind one
    [(0, 0), (-1, 1)],                                  # deletion newest
    [(-1, 1), (-2, 0), (-3, 1)],                        # deletion in the middle
    [(-1, 1), (-2, 1), (-3, 0)],                        # deletion oldest
    [(-1, 7), (-1, 1), (-1, 0), (-2, 1)],               # one sequence, three type bytes
    [(3, 2), (2, 0x7f), (1, 0xff)],                     # nothing parsable at all
    [(-6, 2)],                                          # alone
    "tie", "tie_unparsable",
]


def _chains(rng, S: int, users, over: bool):
    """[(user, seq, type, tie)]: the patterns on the first users, random chains
    on the rest.  ``over`` (wide cases): parsable versions may lie above S, and
    a tie may be unparsable.  In a repair case the second entry of a tie must
    be one the compaction drops, a parsable one at or under S: lcdb's builder
    asserts that the keys it is given strictly increase."""
    out = []
    for i, u in enumerate(users):
        if i < len(PATTERNS):
            p = PATTERNS[i]
            if p == "tie":
                out += [(u, S - 1, 1, True), (u, S - 2, 1, False)]
            elif p == "tie_unparsable":
                out += [(u, S - 1, 1, False), (u, S - 3, 1, False)] if not over else [(u, S - 1, 1, False), (u, S - 2, 7, True), (u, S - 3, 1, False)]
            else:
                out += [(u, S + o, t, False) for o, t in p]
            continue
        seen = set()
        for _ in range(rng.choice((1, 1, 2, 3, 4, 6))):
            t = rng.choice((0, 1, 1, 1, 1, 2, 0x7f, 0xff))
            o = rng.randrange(-9, 4 if (t > 1 or over) else 1)
            if (o, t) not in seen:
                seen.add((o, t))
                out.append((u, S + o, t, rng.random() < 0.05 and (t <= 1 or over)))
    return out


def _deal(rng, versions, ntables: int):
    tables = [[] for _ in range(ntables)]
    for n, (u, seq, typ, tie) in enumerate(versions):
        where = rng.sample(range(ntables), min(2 + (n % 2), ntables) if tie else 1)
        for t in where:
            tables[t].append((ikey(u, seq, typ), b"t%d#%d" % (t, n)))
    return tables


def _edged(tables, S: int, lo: bytes, hi: bytes, typ: int = 1):
    """Every table between a parsable entry of `lo` and one of `hi`; table 0's
    `hi` carries S, the largest parsable sequence, and table 1's S - 1: a
    script that writes `hi` first after its snapshot completes S - 1, S, S + 1."""
    out = []
    for t, es in enumerate(tables):
        es = es + [(ikey(lo, S - 11 - t, typ), b"lo%d" % t),
                   (ikey(hi, S - t if t < 2 else S - 21 - t, typ), b"hi%d" % t)]
        es = isorted(es)
        assert sim_merge.parsable(es[0][0]) and sim_merge.parsable(es[-1][0])
        assert all(sim_merge.compare(a[0], b[0], True) < 0 for a, b in zip(es, es[1:]))
        out.append(es)
    assert max_parsable(out) == S
    return out


def _worked():
    def e(u, s, t, v):
        return (ikey(u, s, t), v)
    return [[e(b"a-lo", 1, 1, b"lo5"), e(b"k", 5, 1, b"k5"), e(b"z-hi", 2, 1, b"hi5")],
            [e(b"a-lo", 3, 1, b"lo7"), e(b"k", 4, 7, b"k4"), e(b"k", 3, 1, b"k3"),
             e(b"m", 9, 2, b"m9"), e(b"m", 8, 1, b"m8"), e(b"m", 7, 1, b"m7"),
             e(b"z-hi", 6, 1, b"hi7")]]


def _types(S: int, seed: int, ntables: int, nusers: int):
    rng = random.Random(seed)
    users = [b"k%03d" % i for i in range(nusers)]
    rng.shuffle(users)
    return _edged(_deal(rng, _chains(rng, S, users, False), ntables), S, b"a-lo", b"z-hi")


def _binary(S: int, seed: int, ntables: int, nusers: int):
    """User keys of a, 00 and ff bytes: the empty key, keys that agree in their
    first 8 and 16 bytes and prefixes padded with 00.  The lowest (the empty
    key) and the highest carry the tables' edges and parsable versions only."""
    rng = random.Random(seed)
    users = binary_users(rng, nusers)
    lo, hi = users[0], users[-1]
    assert lo == b""
    inner = users[1:-1]
    rng.shuffle(inner)
    vs = _chains(rng, S, inner, False) + [(lo, S - 5, 0, False), (lo, S - 6, 1, False),
                                          (hi, S - 1, 0, False), (hi, S - 2, 1, False)]
    return _edged(_deal(rng, vs, ntables), S, lo, hi)


def _unequal(S: int, seed: int, n: int):
    rng = random.Random(seed)
    users = [b"u%05d" % i for i in range(n)]
    vs = _chains(rng, S, users[:40], False) + [(u, S - 1 - i % 7, 1, False)
                                               for i, u in enumerate(users[40:])]
    big = _edged(_deal(rng, vs, 1), S, b"a-lo", b"z-hi")[0]
    mid = users[n // 2]
    return [big, [(ikey(mid, S - 9, 1), b"the one")]]


def _longchain(S: int, seed: int):
    """One user key with 180 versions in two repaired tables at S - 179 .. S
    (deletions and unparsable ones among them, and unparsable ones above S);
    the script adds more above the snapshot."""
    rng = random.Random(seed)
    vs = []
    for o in range(180):
        t = 0 if o in (60, 61, 179) else 7 if o in (50, 51, 100) else 1
        vs.append((b"chain", S - o, t, False))
    vs += [(b"chain", S + 30, 0xff, False), (b"chain", S + 31, 2, False),
           (b"chain", S + 400, 0x7f, False)]
    vs += _chains(rng, S, [b"b%03d" % i for i in range(90)] + [b"d%03d" % i for i in range(60)],
                  False)
    tables = _deal(rng, vs, 2)
    # S itself belongs to the chain, so the edges stay under it.
    edged = []
    for t, es in enumerate(tables):
        es = isorted(es + [(ikey(b"a-lo", S - 211 - t, 1), b"lo%d" % t),
                           (ikey(b"z-hi", S - 221 - t, 1), b"hi%d" % t)])
        edged.append(es)
    assert max_parsable(edged) == S
    return edged


def _allgone(S: int, seed: int):
    """Every user key's newest version is a deletion at or under S: a base-level
    compaction without a snapshot keeps nothing.  The edges are deletions too."""
    rng = random.Random(seed)
    vs = []
    for i in range(120):
        u = b"g%03d" % i
        vs.append((u, S - 1 - i % 5, 0, i % 9 == 0))
        vs += [(u, S - 7 - j, rng.randrange(2), False) for j in range(i % 4)]
    return _edged(_deal(rng, vs, 3), S, b"a-lo", b"z-hi", typ=0)


def _lift(S0: int):
    """One repaired table above the script's key range, so that the script's
    flushed files still land at levels 2, 1, 0 and 0: its entry at S0 lifts
    lcdb's sequences, and the one at S0 - 1 tells a snapshot at S0 from one under it."""
    return [[(ikey(b"~lift", S0, 1), b"lift"), (ikey(b"~lift", S0 - 1, 1), b"lift, older")]]


def _wide(k: int, S: int, seed: int, nusers: int):
    rng = random.Random(seed)
    users = [b"w%04d" % i for i in range(nusers)] + binary_users(rng, nusers // 2)
    rng.shuffle(users)
    vs = _chains(rng, S, users, True)
    # One internal key in every table, parsable and not: the tie order over k runs.
    tables = _deal(rng, vs, k)
    for t in range(k):
        tables[t] += [(ikey(b"everywhere", S, 1), b"run%d" % t),
                      (ikey(b"everywhere", S - 1, 0x7f), b"run%d" % t),
                      (ikey(b"everywhere", S - 2, 0), b"run%d" % t)]
    tables[0] += [(ikey(b"chain", S + 3 - o, 0 if o % 97 == 5 else 7 if o % 89 == 3 else 1),
                   b"c%d" % o) for o in range(0, LONG_CHAIN, 2)]
    tables[k - 1] += [(ikey(b"chain", S + 3 - o, 1), b"c%d" % o) for o in range(1, LONG_CHAIN, 2)]
    return [isorted(t) for t in tables]


_FAMILIES = {"worked": _worked, "types": _types, "binary": _binary, "unequal": _unequal,
             "longchain": _longchain, "allgone": _allgone, "lift": _lift, "wide": _wide}


@functools.lru_cache(maxsize=None)
def _tables(family: str, args: tuple):
    return _FAMILIES[family](*args)


def tables(c: Case) -> list:
    """The case's tables: sorted (internal key, value) lists.  Shared, not to be changed."""
    return _tables(c.family, c.args)


# ---- scripts ---------------------------------------------------------------------

def script(c: Case):
    """(flushed files' entries, smallest_snapshot, last sequence) of a repair
    case: a write takes the next sequence after the largest parsable one in
    the tables, a snapshot holds the last one written, and a flush writes the
    memtable's entries, every version, in the comparator's order."""
    seq = max_parsable(tables(c))
    snap, mem, flushed = None, [], []
    for op in c.ops:
        if op[0] == "p":
            seq += 1
            mem.append((ikey(op[1], seq, 1), op[2]))
        elif op[0] == "d":
            seq += 1
            mem.append((ikey(op[1], seq, 0), b""))
        elif op[0] == "f":
            flushed.append(isorted(mem))
            mem = []
        else:
            snap = seq if snap is None else snap
    assert not mem and seq <= MAX_SEQUENCE
    return flushed, (seq if snap is None else snap), seq


def sources(c: Case) -> dict:
    """{"t<i>" / "f<i>": entries} of a repair case."""
    out = {"t%d" % i: t for i, t in enumerate(tables(c))}
    out.update({"f%d" % i: f for i, f in enumerate(script(c)[0])})
    return out


def _after_snapshot(users, n: int, tail=(), first: bytes = b"z-hi"):
    """A snapshot, then writes on `users` (every fifth a deletion), the edges
    among them so that the flushed file overlaps the tables and stays at level
    0, then the flush.  The first write, one over the snapshot, is on `first`."""
    ops = [("s",), ("p", first, b"first, late"), ("p", b"z-hi", b"hi, late")]
    for i in range(n):
        u = users[i % len(users)]
        ops.append(("d", u) if i % 5 == 4 else ("p", u, b"late%d" % i))
    return tuple(ops + list(tail) + [("p", b"a-lo", b"lo, late"), ("f",)])


def _groups():
    """The four flushed groups of tests/golden/make_merge_golden.py's
    scenarios, which land at levels 2, 1, 0 and 0, with `k1` written last in
    every group (twice) and first in the next: versions of one user key at the
    snapshot, one under and one over, whichever group the snapshot follows.
    The first write of all is a deletion: one over a snapshot taken before
    everything, where only the deletion clause can tell."""
    def edge(g):
        return [("p", b"a-lo", b"lo%d" % g), ("p", b"z-hi", b"hi%d" % g)]

    def k1(g, n):
        return [("p", b"k1", b"v1.%d.%d" % (g, i)) for i in range(n)]

    fill = [("p", b"fill%03d" % i, b"f" * (i % 50)) for i in range(60)]
    return [
        [("d", b"gone")] + edge(1) + fill + [("p", b"k2", b"v2a"), ("p", b"d1", b"x1"),
                                             ("p", b"d3", b"x3")] + k1(1, 2),
        k1(2, 1) + edge(2) + [("p", b"d2", b"y2"), ("d", b"d3"), ("p", b"k4", b"")] + k1(2, 2),
        k1(3, 1) + edge(3) + [("d", b"d1"), ("p", b"d3", b"x3again"), ("p", b"k4", b"v4c"),
                              ("d", b"k4"), ("d", b"k1")] + k1(3, 2),
        k1(4, 1) + edge(4) + [("p", b"k3", b"v3d"), ("d", b"d2"), ("d", b"never")] + k1(4, 2),
    ]


def _lifted_ops(where):
    ops = [("s",)] if where == 0 else []
    for g, grp in enumerate(_groups(), 1):
        ops += grp + [("f",)]
        if where == g:
            ops.append(("s",))
    return tuple(ops)


# ---- the cases ---------------------------------------------------------------------

def L_REPAIR(n: int):
    return ((n, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0))


L_NOTHING = ((3, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0))
L_LIFTED = ((3, 1, 1, 0), (0, 1, 1, 0), (0, 0, 1, 0))


@functools.lru_cache(maxsize=1)
def all_cases():
    out = [Case("worked_example", "repair", "worked", (), (), L_REPAIR(2))]
    k = [b"k%03d" % i for i in range(40)]
    for j, S in enumerate(S_EDGES):
        # No snapshot: smallest_snapshot is the last sequence, S.
        out.append(Case(f"types/S{S:#x}/no_snapshot", "repair", "types", (S, 10 + j, 2 + j % 2, 90),
                        (), L_REPAIR(2 + j % 2)))
        # A snapshot at S, then writes at S + 1 ..: at 2^56 - 4 three of them.
        ops = _after_snapshot(k, 60) if S + 70 < MAX_SEQUENCE else \
            (("s",), ("p", b"z-hi", b"late"), ("p", b"k001", b"late"), ("d", b"a-lo"), ("f",))
        out.append(Case(f"types/S{S:#x}/snapshot", "repair", "types", (S, 20 + j, 2, 90), ops,
                        L_REPAIR(3)))
    for j, S in enumerate((S_EDGES[0], S_EDGES[3], S_EDGES[5])):
        out.append(Case(f"binary/S{S:#x}/no_snapshot", "repair", "binary", (S, 30 + j, 3, 150),
                        (), L_REPAIR(3)))
    bu = tables(Case("", "repair", "binary", (S_EDGES[2], 40, 2, 150)))
    late = sorted({e[0][:-8] for t in bu for e in t})[:30]
    out.append(Case(f"binary/S{S_EDGES[2]:#x}/snapshot", "repair", "binary",
                    (S_EDGES[2], 40, 2, 150),
                    (("s",), ("p", bu[0][-1][0][:-8], b"hi, late")) +
                    tuple(("d", u) if i % 4 == 3 else ("p", u, b"late%d" % i)
                          for i, u in enumerate(late)) + (("f",),), L_REPAIR(3)))
    out.append(Case("unequal/one_against_3000", "repair", "unequal", (S_EDGES[4], 50, 3000), (),
                    L_REPAIR(2)))
    out.append(Case("longchain/snapshot_inside", "repair", "longchain", (S_EDGES[2], 60),
                    _after_snapshot([b"chain"], LONG_CHAIN - 180,
                                    tail=[("d", b"chain"), ("p", b"chain", b"newest")],
                                    first=b"chain"),
                    L_REPAIR(3)))
    out.append(Case("allgone/no_output_file", "repair", "allgone", (S_EDGES[1], 70), (), L_NOTHING))
    for S0, (name, where) in zip(S_EDGES, (("no_snapshot", None), ("snapshot_before_all", 0),
                                           ("snapshot_after_group1", 1),
                                           ("snapshot_after_group2", 2),
                                           ("snapshot_after_group3", 3))):
        out.append(Case(f"lifted/S{S0:#x}/{name}", "repair", "lift", (S0,), _lifted_ops(where),
                        L_LIFTED))
    for j, kk in enumerate((2, 3, 17, 33, 64)):
        S = S_EDGES[(2, 3, 4, 5, 1)[j]]             # not 2^8 - 1: the long chain lies under S
        out.append(Case(f"wide/k{kk}/S{S:#x}", "wide", "wide", (kk, S, 80 + j, 160),
                        snapshots=(0, S - 1, S, S + 1, S + 2, MAX_SEQUENCE)))
    assert len({c.name for c in out}) == len(out)
    return out


# ---- the recorded steps' inputs -----------------------------------------------------

def step_runs(c: Case, steps) -> list:
    """[[entries per input]] per recorded step (merge_sweep_golden_io.Step), in
    lcdb's input order.  "o0" is what the model keeps in the first step;
    test_merge_sweep_sim.py holds that to lcdb's count and digest."""
    src, out = dict(sources(c)), []
    for s in steps:
        out.append([src[n] for n in s.inputs])
        if "o0" not in src:
            src["o0"] = sim_merge.merge(out[-1], True, True, s.smallest_snapshot,
                                        bool(s.drop_deletions))[0]
    return out
