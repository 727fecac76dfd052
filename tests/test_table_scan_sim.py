"""tools/sim_table_scan.py (no GPU): its plain-Python forward scan reproduces
what lcdb's own table iterator delivered for every run of
tests/golden/table_scan.bin, and the formulations the device code uses (key
rebuilding by links, the speculative index parse, the windowed scan) equal
the serial restatement."""
from __future__ import annotations

import os
import random
import struct
import sys

import damage_golden_io as dio
import table_get_golden_io as ggio
import table_golden_io
import table_io
import table_scan_golden_io as gio

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_table_get as simget  # noqa: E402
import sim_table_scan as sim  # noqa: E402

_SETS = table_golden_io.read()
_CASES = gio.read()


def _table(c):
    return simget.Table(gio.table_of(c, _SETS), bool(c.paranoid), bool(c.internal),
                        simget.FILTER_NAME if c.bits_per_key else None)


def _check(c, r, st, ents):
    what = (c.name, None if r.start is None else r.start[:24])
    assert table_io.same_outcome(st, r.rc), what + (st, r.rc)
    assert len(ents) == r.count, what + (len(ents), r.count)
    assert sim.digest(ents) == r.digest, what
    if r.entries is not None:
        assert ents == r.entries, what


def test_fixture_covers_the_issue_cases():
    assert os.path.getsize(gio.PATH) < 512 * 1024
    plain = {(c.set_name, c.variant) for c in _CASES if not c.patches}
    assert plain == {(s.name, i) for s in _SETS for i in range(len(s.variants))}
    names = {c.name.split(":", 1)[1] for c in _CASES if c.patches}
    assert {g.name.split(":", 1)[1] for g in ggio.read() if g.patches} <= names
    for want in ("damage_before_later_restart", "restart_slot0_not_0", "damage_in_last_block",
                 "index_slot_repeated", "index_seek_off_walk"):
        assert want in names, want
    for c in _CASES:
        assert c.open_rc == table_io.LDB_OK
        assert len(c.runs) >= 4 and c.runs[0].start is None
        assert all(r.start is not None for r in c.runs[1:])
    # Where a forward walk and a seek differ: the full scan ends in an error
    # that a seek into a later restart run of the same block does not meet.
    c = next(c for c in _CASES if c.name == "fill4096:damage_before_later_restart")
    assert c.runs[0].rc != 0 and any(r.rc == 0 and r.count for r in c.runs[1:])
    assert any(r.entries is not None and r.count for c in _CASES for r in c.runs)


def test_scan_reproduces_every_fixture_run():
    n = 0
    for c in _CASES:
        t = _table(c)
        for r in c.runs:
            st, ents = sim.scan(t, bool(c.verify), r.start)
            _check(c, r, st, ents)
            n += 1
    assert n > 400


def test_scan_reproduces_every_damage_run():
    """The damaged tables: open status, then sim.scan and the windowed scan at
    windows of 1, 7 and everything against every recorded run."""
    n = 0
    for c in dio.read_scan():
        t = _table(c)
        assert table_io.same_outcome(t.status, c.open_rc), (c.name, t.status, c.open_rc)
        if c.open_rc:
            assert sim.scan(t, bool(c.verify)) == (t.status, [])
            assert sim.scan_windows(t, bool(c.verify), None, 7) == (t.status, [])
        for r in c.runs:
            _check(c, r, *sim.scan(t, bool(c.verify), r.start))
            for w in (1, 7, 1 << 20):
                _check(c, r, *sim.scan_windows(t, bool(c.verify), r.start, w))
            n += 1
    assert n > 200


def test_unpatched_scan_is_the_entry_list():
    for c in _CASES:
        if c.patches:
            continue
        s = next(x for x in _SETS if x.name == c.set_name)
        st, ents = sim.scan(_table(c), True)
        assert st == sim.ST_OK and ents == list(s.entries), c.name


def test_windowed_scan_reproduces_every_fixture_run():
    """lgs_table_scan's route (index entry list, windows, a seek's first block
    walked in the seek's restart run) for windows of 1, 2, 7 blocks and of
    everything."""
    for c in _CASES:
        t = _table(c)
        for r in c.runs:
            for w in (1, 2, 7, 1 << 20):
                st, ents = sim.scan_windows(t, bool(c.verify), r.start, w)
                _check(c, r, st, ents)


def test_end_cut_is_a_prefix_in_order():
    for c in _CASES[::7]:
        t = _table(c)
        st, full = sim.scan(t, bool(c.verify))
        if len(full) < 3:
            continue
        for end in (full[len(full) // 2][0], full[0][0], full[-1][0] + b"\xff" * 9, b""):
            if c.internal and len(end) < 8:
                continue
            cut = next((i for i, (k, _) in enumerate(full)
                        if simget.compare(k, end, bool(c.internal)) >= 0), len(full))
            _, got = sim.scan_windows(t, bool(c.verify), None, 3, end)
            assert got == full[:cut], c.name


def _blocks():
    for s in _SETS:
        internal = s.name.endswith("_internal")
        for v in s.variants:
            for b in v.blocks:
                yield b, internal


def test_link_rebuilding_equals_the_buffer_walk():
    rng = random.Random(1234)
    n = damaged = 0
    for b, internal in _blocks():
        assert sim.block_walk_links(b, internal) == sim.block_walk(b, internal)
        n += 1
    pool = [x for x in _blocks()][::max(1, n // 60)]
    for b, internal in pool:
        for _ in range(6):
            d = bytearray(b)
            for _ in range(rng.choice([1, 1, 2, 5])):
                at = rng.randrange(len(d))
                d[at] = rng.choice([0, 1, 7, 8, 0x7f, 0x80, 0xff, d[at] ^ (1 << rng.randrange(8))])
            d = bytes(d)
            assert sim.block_walk_links(d, internal) == sim.block_walk(d, internal)
            st, heads = sim._headers(d, internal, None)
            if heads:
                wf = rng.choice(heads)[0]
                ef = rng.choice([h[0] for h in heads if h[0] >= wf])
                assert (sim.block_walk_links(d, internal, wf, ef) ==
                        sim.block_walk(d, internal, wf, ef))
            damaged += 1
    assert n > 100 and damaged >= 300
    # The hostile block of the issue: one key, then entries with shared = 1.
    blk = hostile_block(2000)
    st, es = sim.block_walk_links(blk)
    assert st == sim.ST_OK and len(es) == 2000 and es == sim.block_walk(blk)[1]
    import sim_block_cut
    e = ggio.version_entries()
    (vb,) = sim_block_cut.serial_blocks(e, 1 << 20, 16)[1]
    assert [(k, v) for _, k, v in sim.block_walk_links(vb, True)[1]] == e


def hostile_block(n: int) -> bytes:
    """One restart, one 40-byte key, then n - 1 entries with shared = 1."""
    out = bytes([0, 40, 1]) + b"k" * 40 + b"v"
    for i in range(1, n):
        out += bytes([1, 2, 1]) + struct.pack("<H", i) + b"w"
    return out + struct.pack("<II", 0, 1)


def test_speculative_index_parse_equals_the_serial_walk():
    fell = set()
    for c in _CASES:
        t = _table(c)
        if t.index is None:
            continue
        st, ents, fb = sim.index_entries(t.index, bool(c.internal))
        wst, want = sim.index_walk_serial(t.index, bool(c.internal))
        assert (st, ents) == (wst, want), c.name
        if fb:
            fell.add(c.name.split(":", 1)[1])
        if not c.patches:
            assert not fb, c.name
    assert {"index_slot_repeated", "index_seek_off_walk"} <= fell
