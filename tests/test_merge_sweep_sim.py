"""tools/sim_merge.py (and sim_table_split.py for the files) against what
lcdb's own compaction loop kept and wrote for the generated sweep
(tests/merge_sweep.py, tests/golden/merge_sweep.bin), and the sweep against
the edges it is there for.  The edge assertions are computed from the
generated inputs, the records and the model, never from the code under test.
No GPU: test_gpu_merge_sweep.py holds the kernels to the same records."""
from __future__ import annotations

import hashlib
from itertools import groupby

import pytest

import merge_sweep as sweep
import merge_sweep_golden_io as gio
from merge_helpers import ikey

import sim_merge as sim  # noqa: E402
import sim_table_split  # noqa: E402

RECORDS = gio.read()
CASES = {c.name: c for c in sweep.all_cases()}
REPAIR = [r for r in RECORDS if r.kind == "repair"]
WIDE = [r for r in RECORDS if r.kind == "wide"]
STEPS = [(r, s, runs) for r in REPAIR
         for s, runs in zip(r.steps, sweep.step_runs(CASES[r.name], r.steps))]


def seq_of(k: bytes) -> int:
    return sim.tag_of(k) >> 8


def merged_keys(runs):
    return [k for k, _ in sim.merge(runs, True)[0]]


def chains(keys):
    """[[key]] per run of one user key in a merged order."""
    return [list(g) for _, g in groupby(keys, key=lambda k: k[:-8])]


def test_records_are_the_case_list():
    assert [c.name for c in sweep.all_cases()] == [r.name for r in RECORDS]
    for r in RECORDS:
        c = CASES[r.name]
        assert r.kind == c.kind
        if c.kind == "wide":                           # the generator is stable
            assert r.sources == [("t%d" % i, len(t), gio.digest(t))
                                 for i, t in enumerate(sweep.tables(c))]
        else:
            src = sweep.sources(c)
            assert r.sources == [(n, len(es), gio.digest(es)) for n, es in sorted(src.items())]
            _, smallest, _ = sweep.script(c)
            assert r.steps and all(s.smallest_snapshot == smallest for s in r.steps)
            assert sum(len(es) for es in src.values()) <= 4000


@pytest.mark.parametrize("r,s,runs", STEPS, ids=[s.name for _, s, _ in STEPS])
def test_model_reproduces_every_step(r, s, runs):
    dd = bool(s.drop_deletions)
    kept, src, dropped = sim.merge(runs, True, True, s.smallest_snapshot, dd)
    assert (len(kept), gio.digest(kept)) == (s.count, s.digest)
    if s.entries is not None:
        assert kept == s.entries
    assert dropped == sum(len(x) for x in runs) - s.count
    assert [runs[a][i] for a, i in src] == kept
    keys = merged_keys(runs)
    assert sim.drop_flags(keys, s.smallest_snapshot, dd) == \
        sim.drop_serial(keys, s.smallest_snapshot, dd)
    if s.out_bytes is None:
        assert s.count == 0
    else:
        _, (img,) = sim_table_split.split_serial(kept, *sweep.OPTIONS, True)
        assert (len(img), hashlib.sha256(img).digest()) == (s.out_bytes, s.out_sha256)


@pytest.mark.parametrize("r", WIDE, ids=lambda r: r.name)
def test_model_reproduces_every_wide_merge(r):
    c = CASES[r.name]
    ts = sweep.tables(c)
    got, order, _ = sim.merge(ts, True)
    assert (len(got), gio.digest(got)) == (r.count, r.digest)
    if r.entries is not None:
        assert got == r.entries
    assert order == sim.merge_serial(ts, True)
    keys = [k for k, _ in got]
    for snap in c.snapshots:
        for dd in (False, True):
            flags = sim.drop_flags(keys, snap, dd)
            assert flags == sim.drop_serial(keys, snap, dd)
            assert not any(f for f, k in zip(flags, keys) if not sim.parsable(k))


def test_the_worked_example():
    """Two repaired tables, no snapshot: lcdb keeps (k,4,7), the "error key",
    and (k,3,1) behind it."""
    r = next(r for r in RECORDS if r.name == "worked_example")
    s = r.steps[0]
    assert (s.inputs, s.smallest_snapshot, s.drop_deletions) == (["t1", "t0"], 8, 1)
    assert CASES[r.name].snapshots == () and sweep.MAX_SEQUENCE == sim.MAX_SEQUENCE
    assert [k for k, _ in s.entries] == [ikey(b"a-lo", 3, 1), ikey(b"k", 5, 1), ikey(b"k", 4, 7),
                                         ikey(b"k", 3, 1), ikey(b"m", 9, 2), ikey(b"m", 8, 1),
                                         ikey(b"z-hi", 6, 1)]
    runs = sweep.step_runs(CASES[r.name], r.steps)[0]
    assert sim.merge(runs, True, True, 8, True)[0] == s.entries
    assert r.steps[1].inputs == ["o0"] and r.steps[1].entries == s.entries


def test_every_case_has_a_witness_for_its_snapshot():
    """The kept entries of some step change when smallest_snapshot is one
    lower, and, where the script wrote above its snapshot, of some step when
    it is one higher: a snapshot the recipe computed wrongly cannot pass."""
    for r in REPAIR:
        c = CASES[r.name]
        _, smallest, last = sweep.script(c)
        lower = upper = False
        for s, runs in zip(r.steps, sweep.step_runs(c, r.steps)):
            dd = bool(s.drop_deletions)
            kept = sim.merge(runs, True, True, smallest, dd)[0]
            lower |= sim.merge(runs, True, True, smallest - 1, dd)[0] != kept
            upper |= sim.merge(runs, True, True, smallest + 1, dd)[0] != kept
        assert lower and (upper or last == smallest), r.name


# ---- the sweep reaches the edges ------------------------------------------------

def test_type_bytes():
    seen, where, rows, rel = set(), set(), 0, set()
    behind_dropped = 0
    for _, s, runs in STEPS:
        keys = merged_keys(runs)
        flags = sim.drop_flags(keys, s.smallest_snapshot, bool(s.drop_deletions))
        drop = dict(zip(range(len(keys)), flags))
        at = 0
        for ch in chains(keys):
            for i, k in enumerate(ch):
                if sim.parsable(k):
                    if i and not sim.parsable(ch[i - 1]) and k[-8] == 0 and \
                            seq_of(k) <= s.smallest_snapshot and s.drop_deletions:
                        assert drop[at + i]
                        behind_dropped += 1
                    continue
                seen.add(k[-8])
                assert not drop[at + i]
                if len(ch) > 2:
                    where.add("newest" if i == 0 else "oldest" if i == len(ch) - 1 else "middle")
                rows += i > 0 and not sim.parsable(ch[i - 1])
                q = seq_of(k)
                rel.add("under" if q < s.smallest_snapshot else
                        "over" if q > s.smallest_snapshot else "equal")
            at += len(ch)
    assert seen >= {2, 0x7f, 0xff}
    assert where == {"newest", "middle", "oldest"}
    assert rows >= 3 and rel == {"under", "equal", "over"} and behind_dropped >= 3
    # drop_deletions = 0 with unparsable keys is not reachable through a
    # repair: the wide cases hold it, on lcdb's order and the model's rule.
    behind_kept = 0
    for r in WIDE:
        c = CASES[r.name]
        keys = merged_keys(sweep.tables(c))
        assert {k[-8] for k in keys} >= {0, 1, 2, 0x7f, 0xff}
        for snap in c.snapshots[:-1]:               # at MAX_SEQUENCE rule (A) drops first occurrences too
            flags = sim.drop_flags(keys, snap, False)
            for i in range(1, len(keys)):
                if keys[i][:-8] == keys[i - 1][:-8] and not sim.parsable(keys[i - 1]) and \
                        keys[i][-8] == 0 and seq_of(keys[i]) <= snap:
                    assert not flags[i] and sim.drop_flags(keys, snap, True)[i]
                    behind_kept += 1
    assert behind_kept >= 3


def test_sequences_and_snapshots():
    tops = {sweep.max_parsable(sweep.tables(CASES[r.name])) for r in REPAIR}
    assert tops >= set(sweep.S_EDGES)
    # Parsable versions of one user key at the snapshot, one under and one
    # over, in every case whose snapshot has writes on both sides.
    around = set()
    for r, s, runs in STEPS:
        for ch in chains(merged_keys(runs)):
            seqs = {seq_of(k) for k in ch if sim.parsable(k)}
            if {s.smallest_snapshot - 1, s.smallest_snapshot, s.smallest_snapshot + 1} <= seqs:
                around.add(r.name)
    want = {r.name for r in REPAIR if ("s",) in CASES[r.name].ops and
            not r.name.endswith("snapshot_before_all")}     # there only `~lift` lies under it
    assert len(want) >= 11 and around >= want
    held = {r.name: any(op == ("s",) for op in CASES[r.name].ops) for r in REPAIR}
    assert sum(held.values()) >= 5 and sum(not h for h in held.values()) >= 5
    # A snapshot before everything the script writes, with both drop_deletions.
    r = next(r for r in REPAIR if r.name.endswith("snapshot_before_all"))
    c = CASES[r.name]
    assert c.ops[0] == ("s",)
    assert all(seq_of(k) > r.steps[0].smallest_snapshot
               for n, es in sweep.sources(c).items() if n[0] == "f" for k, _ in es)
    assert {s.drop_deletions for s in r.steps} == {0, 1}
    lifted = [s for r in REPAIR if r.name.startswith("lifted") for s in r.steps]
    assert {(s.drop_deletions, s.smallest_snapshot >> 32 > 0) for s in lifted} == \
        {(d, b) for d in (0, 1) for b in (False, True)}
    assert max(sweep.script(CASES[r.name])[2] for r in REPAIR) == sweep.MAX_SEQUENCE


def test_user_keys():
    users = {k[:-8] for r in REPAIR for t in sweep.tables(CASES[r.name]) for k, _ in t}
    assert b"" in users
    by8, by16 = {}, {}
    for u in users:
        if len(u) > 8:
            by8.setdefault(u[:8], set()).add(u)
        if len(u) > 16:
            by16.setdefault(u[:16], set()).add(u)
    assert any(len(v) > 2 and len({u[:9] for u in v}) > 1 for v in by8.values())
    assert any(len(v) > 1 for v in by16.values())
    assert sum(u + b"\0" in users for u in users) >= 3
    assert sum(u + b"\0\0" in users or (u + b"\0" in users and u[-1:] == b"\0") for u in users) >= 1


def test_version_chains():
    long_, dels = 0, set()
    for _, s, runs in STEPS:
        keys = merged_keys(runs)
        at = 0
        for ch in chains(keys):
            if len(ch) > 256:
                above = sum(seq_of(k) > s.smallest_snapshot for k in ch)
                spread = sum(any(k[:-8] == ch[0][:-8] for k, _ in r) for r in runs)
                assert 0 < above < len(ch) and spread >= 2
                assert at // 256 != (at + len(ch) - 1) // 256     # over a workgroup's edge
                long_ += 1
            if len(ch) > 2 and all(sim.parsable(k) for k in ch):
                for i, k in enumerate(ch):
                    if k[-8] == 0:
                        dels.add("newest" if i == 0 else "oldest" if i == len(ch) - 1 else "middle")
            at += len(ch)
    assert long_ >= 1 and dels == {"newest", "middle", "oldest"}
    for r in WIDE:
        keys = merged_keys(sweep.tables(CASES[r.name]))
        assert max(len(ch) for ch in chains(keys)) >= sweep.LONG_CHAIN


def test_input_shapes():
    ties = 0
    for _, s, runs in STEPS:
        where = {}
        for j, run in enumerate(runs):
            for k, v in run:
                where.setdefault(k, []).append((j, v))
        ties += sum(len(w) > 1 and len({v for _, v in w}) == len(w) for w in where.values())
    assert ties >= 5
    assert sum(len(s.inputs) == 1 for _, s, _ in STEPS) >= 5
    assert {len(s.inputs) for _, s, _ in STEPS} >= {1, 2, 3, 4}
    assert any(s.count == 0 and s.out_bytes is None and sum(map(len, runs)) > 100
               for _, s, runs in STEPS)
    assert any(sorted(map(len, runs))[0] == 1 and sorted(map(len, runs))[-1] >= 3000
               for _, s, runs in STEPS)
    # Level 0 as lcdb lists it is not always the order the tables were written in.
    assert any(s.inputs[:2] == ["t1", "t0"] for _, s, _ in STEPS)
    assert {len(sweep.tables(CASES[r.name])) for r in WIDE} == {2, 3, 17, 33, 64}
    for r in WIDE:
        ts = sweep.tables(CASES[r.name])
        every = [k for k, _ in ts[0] if all(any(k == q for q, _ in t) for t in ts[1:])]
        assert any(sim.parsable(k) for k in every) and any(not sim.parsable(k) for k in every)


def test_neighbour_form_equals_the_loop_on_random_orders():
    """drop_flags (entries i and i - 1) against drop_serial (lcdb's loop with
    its failed import) on random merged orders with every type byte, at every
    snapshot around their sequences."""
    import random
    rng = random.Random(41)
    for _ in range(300):
        es = {ikey(bytes(rng.choice(b"ab") for _ in range(rng.randrange(3))), rng.randrange(1, 7),
                   rng.choice((0, 1, 1, 2, 0x7f, 0xff))) for _ in range(rng.randrange(1, 25))}
        keys = [k for k, _ in sweep.isorted([(k, b"") for k in es])]
        for snap in range(0, 8):
            for dd in (False, True):
                flags = sim.drop_flags(keys, snap, dd)
                assert flags == sim.drop_serial(keys, snap, dd)
                assert not any(f for f, k in zip(flags, keys) if not sim.parsable(k))
