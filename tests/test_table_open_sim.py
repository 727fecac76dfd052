"""tools/sim_table_get.py's numbering of a batch's distinct blocks (no GPU):
the model of live_mark_kernel, the scan of the marks and qblock_kernel against
a set-based de-duplication, on the fixture's tables and on random subsets of
their queries."""
from __future__ import annotations

import os
import random
import sys

import table_get_golden_io as gio
import table_golden_io
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_table_get as sim  # noqa: E402


def _check(t: sim.Table, keys, verify: bool):
    pre, qblock, nb, handles = sim.number_blocks(t, keys)
    assert len(pre) == len(qblock) == len(keys) and len(handles) == nb
    # The set-based restatement: the distinct entries the live queries found.
    found = [sim.index_lookup(t, k) for k in keys]
    live = sorted({f[2] for f in found if f[4]})
    assert nb == len(live)
    by_entry = {}
    for q, (state, ist, at, h, lv) in enumerate(found):
        if not lv:
            assert qblock[q] == sim.NO_BLOCK
            want = ist if state == 0 else (sim.ST_CORRUPT if state == 2 else sim.ST_OK)
            assert pre[q] == want
            continue
        assert state == 1 and pre[q] == sim.ST_OK
        # No two queries disagree on the block of one entry, and ranks are
        # dense and in file order.
        assert by_entry.setdefault(at, qblock[q]) == qblock[q]
        assert qblock[q] == live.index(at)
        assert handles[qblock[q]] == h
    assert sorted(by_entry.values()) == list(range(nb))
    # The numbering leads to what Table.get returns: a query without a block
    # answers pre[q], one with a block reads the block its number names.
    for q, k in enumerate(keys):
        called, st, _, _ = t.get(k, verify)
        if qblock[q] == sim.NO_BLOCK:
            assert not called and st == pre[q], (q, k[:40])
        else:
            off, size = handles[qblock[q]]
            assert (off, size, verify) in t.blocks
    return nb


def test_numbering_equals_a_set_based_dedup_on_the_fixture():
    rng = random.Random(7)
    sets = table_golden_io.read()
    cases = gio.read()
    tables = blocks = 0
    kinds = set()
    for c in cases:
        # Every patched table, and every fourth plain one (the plain ones
        # differ in size and compression, not in what the numbering sees).
        if not c.patches and tables % 4:
            tables += 1
            continue
        tables += 1
        t = sim.Table(gio.table_of(c, sets), bool(c.paranoid), bool(c.internal),
                      sim.FILTER_NAME if c.bits_per_key else None)
        keys = [r.key for r in c.records]
        blocks += _check(t, keys, bool(c.verify))
        if c.patches:
            kinds.add(c.name.split(":", 1)[1])
        # Query order must not matter, nor which queries share a batch.
        sub = rng.sample(keys, max(1, len(keys) // 3))
        _check(t, sub, bool(c.verify))
        pre, qb, nb, _ = sim.number_blocks(t, keys)
        rpre, rqb, rnb, _ = sim.number_blocks(t, keys[::-1])
        assert (rpre[::-1], rqb[::-1], rnb) == (pre, qb, nb)
    assert blocks > 200 and {"index_value_no_handle", "handle_past_file_end"} <= kinds


def test_entries_with_one_handle_are_two_blocks():
    """The key is the entry's offset: an index block whose two entries carry
    the same handle numbers two blocks (and reads the block twice)."""
    import struct

    def entry(key: bytes, value: bytes) -> bytes:
        return bytes([0, len(key), len(value)]) + key + value

    h = bytes([0, 10])                                     # handle (0, 10)
    e0, e1 = entry(b"b", h), entry(b"d", h)
    index = e0 + e1 + struct.pack("<III", 0, len(e0), 2)
    t = sim.Table(b"")                                     # does not open; filled by hand
    t.index, t.filter, t.status, t.internal = index, None, sim.ST_OK, False
    pre, qblock, nb, handles = sim.number_blocks(t, [b"c", b"a", b"d", b"e"])
    assert qblock == [1, 0, 1, sim.NO_BLOCK] and nb == 2
    assert handles == [(0, 10), (0, 10)] and pre == [sim.ST_OK] * 4


def test_a_table_that_does_not_open_numbers_nothing():
    t = sim.Table(b"short")
    assert sim.number_blocks(t, [b"k1", b"k2"]) == ([sim.ST_CORRUPT] * 2, [sim.NO_BLOCK] * 2, 0, [])
