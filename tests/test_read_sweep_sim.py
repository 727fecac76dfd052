"""The read side's CPU models on the generated sweep:
tools/sim_table_get.py and sim_table_scan.py against what lcdb's own table
reader returned for every target and scan start of tests/read_sweep.py
(tests/golden/read_sweep.bin).  The fixture keeps ordinals only; the entries
and the images are regenerated and checked against their recorded digests
first, so an ordinal stands for lcdb's own key and value bytes."""
from __future__ import annotations

import bisect
import functools
import hashlib

import pytest

import read_sweep as rs
import read_sweep_golden_io as gio
import table_io
from merge_golden_io import digest

import sim_table_get as sim  # noqa: E402  (read_sweep put tools/ on the path)
import sim_table_scan  # noqa: E402

TABLES = rs.tables()
RECORDS = gio.read()
PAIRS = list(zip(TABLES, RECORDS))
IDS = [t.name for t in TABLES]
_CACHE: dict = {}


def pin(t, r):
    return (r.size, r.sha) if t.versions else rs.sweep_pin(t)


def model(t, r):
    """(image, opened model table) of a table, made once for this module."""
    if t.name not in _CACHE:
        img = rs.image(t, pin(t, r))
        _CACHE[t.name] = img, sim.Table(img, False, bool(t.internal),
                                        sim.FILTER_NAME if t.bits_per_key else None)
    return _CACHE[t.name]


def compare_key(t):
    return functools.cmp_to_key(lambda a, b: sim.compare(a, b, bool(t.internal)))


def test_the_fixture_names_the_sweeps_tables():
    assert [(r.name, r.case, r.file) for r in RECORDS] == [(t.name, t.case, t.file) for t in TABLES]
    assert all(r.open_rc == table_io.LDB_OK for r in RECORDS)
    assert all(bool(r.sha) == t.versions for t, r in PAIRS)
    assert all(len(rs.targets(t)) == len(r.rc) <= rs.MAX_TARGETS for t, r in PAIRS)
    assert all(len(rs.starts(t)) == len(r.starts) <= rs.STARTS for t, r in PAIRS)


def test_entry_sets_and_images():
    """Every entry set regenerates to its recorded count and digest, every
    image to its recorded length and SHA-256."""
    seen = set()
    for t, r in PAIRS:
        if t.spec not in seen:
            seen.add(t.spec)
            es = rs.set_entries(t.spec)
            want = (r.count, r.digest) if t.versions else \
                (rs.sweep_records()[t.case].count, rs.sweep_records()[t.case].digest)
            assert (len(es), digest(es)) == want, t.spec
        img, mt = model(t, r)
        assert (len(img), hashlib.sha256(img).digest()) == tuple(pin(t, r)), t.name
        assert mt.status == sim.ST_OK and (mt.filter is not None) == bool(t.bits_per_key), t.name
    assert rs.VERSIONS_SPEC in seen and len(seen) >= 40


@pytest.mark.parametrize("t,r", PAIRS, ids=IDS)
def test_lookups(t, r):
    """Table.get, and block_seek on the raw block that the model's index
    names, equal every recorded lookup."""
    es = rs.entries(t)
    _, mt = model(t, r)
    _, blocks, ikeys = rs.cut(t)
    ck = compare_key(t)
    iks = [ck(k) for k in ikeys]
    for k, rc, fl, o in zip(rs.targets(t), r.rc, r.flags, r.ordinal):
        what = (t.name, k[:40], rc, fl, o)
        called, st, fk, fv = mt.get(k, True)
        assert table_io.same_outcome(st, rc), what + (st,)
        assert called == bool(fl & gio.CALLED), what
        if called:
            assert (fk, fv) == es[o], what
        if t.internal and len(k) < 8:
            assert sim.block_seek(blocks[0], k, True) == (sim.ST_CORRUPT, None), what
            continue
        b = bisect.bisect_left(iks, ck(k))
        st, e = sim.block_seek(blocks[b], k, bool(t.internal)) if b < len(blocks) else (sim.ST_OK, None)
        assert st == sim.ST_OK, what
        if fl & gio.CALLED:
            assert e is not None and (e[1], blocks[b][e[2]:e[2] + e[3]]) == es[o], what
        else:
            assert (e is not None) == bool(fl & gio.REFUSED), what


@pytest.mark.parametrize("t,r", PAIRS, ids=IDS)
def test_scans(t, r):
    """scan_windows in windows of 1 and 64 blocks equals every recorded scan;
    a recorded scan begins at the comparator's bisect of its start."""
    es = rs.entries(t)
    _, mt = model(t, r)
    ck = compare_key(t)
    keys = [ck(k) for k, _ in es]
    for s, (rc, count, o) in zip(rs.starts(t), r.starts):
        what = (t.name, s[:40], rc, count, o)
        assert count == len(es) - o, what
        if rc == table_io.LDB_OK:
            assert o == bisect.bisect_left(keys, ck(s)), what
        else:
            assert count == 0 and t.internal and len(s) < 8, what
        for w in (1, 64):
            st, got = sim_table_scan.scan_windows(mt, True, s, w)
            assert table_io.same_outcome(st, rc), what + (w, st)
            assert got == es[o:], what + (w,)


def test_class_counts():
    """The recipe's conditions, from the committed fixture."""
    n = rs.conditions(TABLES, RECORDS)
    rs.check_conditions(n)
    _CACHE.clear()
