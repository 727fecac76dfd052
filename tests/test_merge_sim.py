"""tools/sim_merge.py against what lcdb's own merging iterator delivered and
what its own compactions wrote (tests/golden/merge.bin), and the drop rule's
invariant on random inputs.  No GPU: the device tests (test_gpu_merge.py) hold
the kernels to this model."""
from __future__ import annotations

import os
import random
import struct
import sys

import pytest

import merge_golden_io as mio
import table_golden_io
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_merge as sim  # noqa: E402

MERGES, STEPS = mio.read()


@pytest.fixture(scope="module")
def sets():
    return table_golden_io.read()


def test_fixture_covers_the_cases():
    names = {c.name for c in MERGES}
    for n in ("alone", "self", "deal3", "deal7", "empty_among", "one_vs_thousands",
              "thousands_vs_one_tie", "value_sizes"):
        assert n in names and n + "_internal" in names
    assert {"prefixes", "ties_by_run", "user_key_prefixes_internal"} <= names
    assert {(s.drop_deletions, s.name.split(":")[0]) for s in STEPS} == {
        (d, n) for d in (0, 1) for n in ("no_snapshot", "snapshot_before_all",
                                         "snapshot_after_group1", "snapshot_after_group2",
                                         "snapshot_after_group3")}


@pytest.mark.parametrize("case", MERGES, ids=lambda c: c.name)
def test_model_equals_the_reference_merge(case, sets):
    runs = [r.entries(sets) for r in case.runs]
    got, src, dropped = sim.merge(runs, bool(case.internal))
    assert dropped == 0 and len(got) == case.count
    assert mio.digest(got) == case.digest
    if case.entries is not None:
        assert got == case.entries
    assert [runs[r][i] for r, i in src] == got
    assert src == sim.merge_serial(runs, bool(case.internal))


@pytest.mark.parametrize("step", STEPS, ids=lambda s: s.name)
def test_model_equals_the_reference_compaction(step):
    runs = [es for _, es in step.inputs]
    got, src, dropped = sim.merge(runs, True, True, step.smallest_snapshot,
                                  bool(step.drop_deletions))
    assert got == step.out_entries
    assert dropped == sum(len(r) for r in runs) - len(step.out_entries)
    keys = [k for k, _ in sim.merge(runs, True)[0]]
    assert sim.drop_flags(keys, step.smallest_snapshot, bool(step.drop_deletions)) == \
        sim.drop_serial(keys, step.smallest_snapshot, bool(step.drop_deletions))


def test_compare_words_is_the_comparator():
    """The word never decides alone between a key and its zero-padded
    extension, and user-key prefixes order by the user key, not by raw bytes."""
    assert sim.compare_words(b"ab", b"ab\0", False) < 0
    assert sim.compare_words(b"", b"\0", False) < 0
    assert sim.compare_words(b"ABCDEFGH", b"ABCDEFGH\0", False) < 0
    a, b = b"ab" + struct.pack("<Q", (5 << 8) | 1), b"ab\x01" + struct.pack("<Q", (1 << 8) | 1)
    assert a > b and sim.compare_words(a, b, True) < 0        # raw bytes say the opposite
    rng = random.Random(5)
    for _ in range(3000):
        internal = rng.random() < 0.5
        ks = []
        for _k in range(2):
            u = bytes(rng.choice(b"a\0\xff") for _ in range(rng.choice([0, 1, 7, 8, 9, 15, 16, 17])))
            ks.append(u + struct.pack("<Q", rng.randrange(4) << 8 | rng.randrange(2))
                      if internal else u)
        assert sim.compare_words(ks[0], ks[1], internal) == sim.compare(ks[0], ks[1], internal)


def random_runs(rng, internal: bool, k: int, sizes=(0, 1, 2, 5, 9)):
    runs, seq = [], 0
    for _ in range(k):
        es = {}
        for _i in range(rng.choice(sizes)):
            u = bytes(rng.choice(b"ab") for _ in range(rng.randrange(0, 4)))
            if internal:
                seq += 1
                key = u + struct.pack("<Q", (seq << 8) | (rng.random() < 0.7))
            else:
                key = u
            es[key] = b"v%d" % len(es)
        runs.append(sorted(es.items(), key=sim.sort_key(internal)))
    return runs, seq


def test_ranks_equal_the_serial_merge_on_random_runs():
    rng = random.Random(11)
    for _ in range(300):
        internal = rng.random() < 0.5
        runs, _ = random_runs(rng, internal, rng.randrange(0, 10))
        assert sim.merge_ranks(runs, internal) == sim.merge_serial(runs, internal)


def test_drop_keeps_every_view_at_or_after_the_smallest_snapshot():
    """For every snapshot s >= smallest_snapshot a reader sees the same value
    per user key before and after the drop.  With drop_deletions only the runs
    themselves are consulted (base level: nothing older below them)."""
    rng = random.Random(23)
    for _ in range(400):
        runs, last = random_runs(rng, True, rng.randrange(1, 6))
        every = [e for r in runs for e in r]
        smallest = rng.randrange(0, last + 2)
        for dd in (False, True):
            kept, _, dropped = sim.merge(runs, True, True, smallest, dd)
            assert dropped == len(every) - len(kept)
            for s in range(smallest, last + 2):
                before, after = sim.visible(every, s), sim.visible(kept, s)
                assert before == after, (smallest, dd, s)
            if not dd:
                # Not base level: a deletion must go on hiding older data below.
                def newest(es, s):
                    best = {}
                    for k, _ in es:
                        q = sim.tag_of(k) >> 8
                        if q <= s and best.get(k[:-8], (-1,))[0] < q:
                            best[k[:-8]] = (q, sim.tag_of(k) & 0xff)
                    return best
                for s in range(smallest, last + 2):
                    assert newest(every, s) == newest(kept, s)


def test_preconditions():
    with pytest.raises(ValueError):
        sim.merge([[(b"b", b""), (b"a", b"")]])
    with pytest.raises(ValueError):
        sim.merge([[(b"short", b"")]], internal_keys=True)
    with pytest.raises(ValueError):
        sim.merge([[]] * 65)
    with pytest.raises(ValueError):
        sim.merge([[(b"a", b"")]], drop=True)
    assert sim.check_runs([[(b"a", b"")], [(b"b", b""), (b"a", b"")], [(b"z", b""), (b"y", b"")]],
                          False) == 1
