"""Forward scans of opened tables on the device: OpenTable.scan,
.scan_window and .scan_dev against what lcdb's own table iterator delivered
(tests/golden/table_scan.bin), and scan followed by build as the identity."""
from __future__ import annotations

import os
import sys
import threading

import numpy as np
import pytest

import damage_golden_io as dio
import table_golden_io
import table_io
import table_scan_golden_io as gio

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_table_get as simget  # noqa: E402
import sim_table_scan as sim  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


@pytest.fixture(scope="module")
def fixture():
    return table_golden_io.read(), gio.read()


def _open_case(tab, c, file, resident):
    return tab.open_table(file if resident else np.frombuffer(file, dtype=np.uint8).copy(),
                          paranoid_checks=bool(c.paranoid), internal_keys=bool(c.internal),
                          filter_name=tab.FILTER_NAME if c.bits_per_key else None,
                          resident=bool(resident))


def _scan(tab, t, **kw):
    """(final status, entries) of OpenTable.scan."""
    out = []
    try:
        for kv in t.scan(**kw):
            out.append(kv)
    except tab.ScanError as e:
        assert e.status == t.scan_status != tab.LGS_ST_OK
    return t.scan_status, out


def _check(c, r, st, ents):
    what = (c.name, None if r.start is None else r.start[:24])
    assert table_io.same_outcome(st, r.rc), what + (st, r.rc)
    assert len(ents) == r.count, what + (len(ents), r.count)
    assert sim.digest(ents) == r.digest, what
    if r.entries is not None:
        assert ents == r.entries, what


def _group_of(c):
    return "patched" if c.patches else ("internal" if c.internal else "bytewise")


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("group", ["bytewise", "internal", "patched", "damaged"])
def test_scan_equals_the_reference(tab, fixture, group, resident):
    """Every run of every fixture case (the full scan and the recorded seeks,
    the flipped-payload cases verified and unverified among them) in one
    window, and the full scan and the first seek a block at a time.
    "damaged": the randomly damaged tables of damage_scan.bin; one that lcdb
    did not open has its open status and no entries."""
    sets, cases = fixture
    n = 0
    for c in (dio.read_scan() if group == "damaged" else cases):
        if group != "damaged" and _group_of(c) != group:
            continue
        with _open_case(tab, c, gio.table_of(c, sets), resident) as t:
            if group == "damaged" and c.open_rc != table_io.LDB_OK:
                assert table_io.same_outcome(t.status, c.open_rc), (c.name, t.status, c.open_rc)
                for w in (4096, 1):
                    assert _scan(tab, t, verify=bool(c.verify), max_blocks=w) == (t.status, []), c.name
                r = t.scan_window(b"k" * 9)
                assert r["at_end"] and r["blocks_done"] == 0 and r["entries"] == [], c.name
                n += 1
                continue
            assert t.status == tab.LGS_ST_OK, c.name
            for i, r in enumerate(c.runs):
                st, ents = _scan(tab, t, start=r.start, verify=bool(c.verify), max_blocks=4096)
                _check(c, r, st, ents)
                if i < 2:
                    st, ents = _scan(tab, t, start=r.start, verify=bool(c.verify), max_blocks=1)
                    _check(c, r, st, ents)
                n += 1
    assert n >= 100


def _windows_equal_the_model(tab, c, file, width):
    """scan_window's own results for every run of case c in windows of
    `width` blocks (wider where a seek's side walk needs it, as the C call
    asks) against sim.scan_window."""
    mt = simget.Table(file, bool(c.paranoid), bool(c.internal), None)
    lst = sim.IndexList(mt)
    with _open_case(tab, c, file, 1) as t:
        for r in c.runs:
            nxt, first = 0, True
            while True:
                start = r.start if first else None
                want = sim.scan_window(mt, lst, bool(c.verify), start, nxt, width)
                if "need_blocks" in want:
                    want = sim.scan_window(mt, lst, bool(c.verify), start, nxt, want["need_blocks"])
                got = t.scan_window(start, nxt, width, bool(c.verify))
                for k in ("entries", "blocks_done", "next_block", "at_end"):
                    assert got[k] == want[k], (c.name, r.start, k)
                assert [int(x) for x in got["block_entry_first"]] == want["block_entry_first"]
                assert [int(x) for x in got["block_status"]] == want["block_status"]
                if want["at_end"]:
                    assert got["index_status"] == want["index_status"]
                    break
                nxt, first = want["next_block"], False


def test_windows_and_next_block(tab, fixture):
    """scan_window's own results: block_entry_first, block_status, next_block
    and at_end for windows of 7 blocks equal the model's."""
    sets, cases = fixture
    for c in cases:
        if c.name not in ("fill256:3", "fill4096:damage_before_later_restart",
                          "fill256:index_seek_off_walk", "fill4096:index_value_no_handle"):
            continue
        _windows_equal_the_model(tab, c, gio.table_of(c, sets), 7)


def test_windows_and_next_block_on_damaged_index_blocks(tab, fixture):
    """The same on the tables of damage_scan.bin whose index block is damaged."""
    sets, _ = fixture
    n = 0
    for c in dio.read_scan():
        if dio.class_of(c) == "index_block" and c.open_rc == table_io.LDB_OK:
            _windows_equal_the_model(tab, c, gio.table_of(c, sets), 7)
            n += 1
    assert n >= 8


@pytest.mark.parametrize("resident", [0, 1])
def test_end_cuts(tab, fixture, resident):
    sets, cases = fixture
    for name in ("fill256:0", "fill256_internal:3", "fill4096:unsorted_scan"):
        c = next(c for c in cases if c.name == name)
        file = gio.table_of(c, sets)
        mt = simget.Table(file, False, bool(c.internal), None)
        _, full = sim.scan(mt, bool(c.verify))
        with _open_case(tab, c, file, resident) as t:
            for end in (full[len(full) // 2][0], full[0][0], full[-1][0] + b"\xff" * 9,
                        full[7][0][:-1] if not c.internal else full[7][0]):
                cut = next((i for i, (k, _) in enumerate(full)
                            if simget.compare(k, end, bool(c.internal)) >= 0), len(full))
                for w in (1, 3, 4096):
                    st, got = _scan(tab, t, end=end, verify=bool(c.verify), max_blocks=w)
                    assert got == full[:cut] and st == tab.LGS_ST_OK, (name, end, w)
                st, got = _scan(tab, t, start=full[3][0], end=end, verify=bool(c.verify))
                _, want = sim.scan_windows(mt, bool(c.verify), full[3][0], 64, end)
                assert got == want, (name, end)


@pytest.mark.parametrize("resident", [0, 1])
def test_table_that_does_not_open_and_the_empty_table(tab, fixture, resident):
    sets, cases = fixture
    file = next(s for s in sets if s.name == "fill256").variants[0].file
    for bad in (file[:40], file[:-8] + b"\0" * 8):
        with tab.open_table(bad if resident else np.frombuffer(bad, dtype=np.uint8).copy(),
                            resident=bool(resident)) as t:
            assert t.status == tab.LGS_ST_CORRUPT
            st, ents = _scan(tab, t)
            assert (st, ents) == (tab.LGS_ST_CORRUPT, [])
            r = t.scan_window(b"k")
            assert r["at_end"] and r["blocks_done"] == 0 and r["entries"] == []
    for s in sets:
        if s.entries:
            continue
        for v in s.variants:
            with tab.open_table(v.file if resident else np.frombuffer(v.file, dtype=np.uint8).copy(),
                                internal_keys=bool(v.internal), resident=bool(resident)) as t:
                assert _scan(tab, t) == (tab.LGS_ST_OK, [])
                assert _scan(tab, t, start=b"a" * 9) == (tab.LGS_ST_OK, [])


@pytest.mark.parametrize("resident", [0, 1])
def test_device_bytes_grow_once_after_the_first_scan(tab, fixture, resident):
    sets, _ = fixture
    s = next(s for s in sets if s.name == "fill256")
    file = s.variants[3].file
    with tab.open_table(file if resident else np.frombuffer(file, dtype=np.uint8).copy(),
                        resident=bool(resident)) as t:
        before = t.info()["device_bytes"]
        t.get([s.entries[0][0]])
        assert t.info()["device_bytes"] == before
        assert _scan(tab, t)[1] == list(s.entries)
        after = t.info()["device_bytes"]
        assert after > before
        assert _scan(tab, t, start=s.entries[5][0])[1] == list(s.entries[5:])
        t.get([s.entries[0][0]])
        assert t.info()["device_bytes"] == after
        assert after - before <= 17 * len(s.variants[3].blocks) + 1024


def test_two_threads_scan_one_handle(tab, fixture):
    sets, _ = fixture
    s = next(s for s in sets if s.name == "fill256_internal")
    out, errs = {}, []

    def work(i, t, start):
        try:
            out[i] = _scan(tab, t, start=start, max_blocks=3 + i)
        except Exception as e:                          # noqa: BLE001
            errs.append(e)

    for resident in (0, 1):
        v = s.variants[1]
        with tab.open_table(v.file if resident else np.frombuffer(v.file, dtype=np.uint8).copy(),
                            internal_keys=True, resident=bool(resident)) as t:
            # The first scans of the handle, at once: the index entry list is
            # built by one of them.
            th = [threading.Thread(target=work, args=(i, t, None)) for i in range(2)]
            th += [threading.Thread(target=work, args=(2, t, s.entries[20][0]))]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert not errs
            assert out[0] == out[1] == (tab.LGS_ST_OK, list(s.entries))
            assert out[2] == (tab.LGS_ST_OK, list(s.entries[20:]))


def test_build_of_scan_is_the_table(tab, fixture):
    """build(scan(table)) == table: one variant of each fixture set per
    compression."""
    sets, _ = fixture
    n = 0
    for s in sets:
        seen = set()
        for v in s.variants:
            if v.compression in seen:
                continue
            seen.add(v.compression)
            with tab.open_table(v.file, internal_keys=bool(v.internal), resident=True) as t:
                ents = list(t.scan())
            assert ents == list(s.entries)
            again = tab.build_table_host(ents, v.block_size, v.restart_interval, v.compression,
                                         v.bits_per_key, bool(v.internal))
            assert again == v.file, (s.name, v.block_size, v.compression)
            n += 1
    assert n >= 35


def test_scan_dev_feeds_build_blocks(tab, fixture):
    """On device tensors: scan_dev's outputs go into build_blocks as they
    stand and give the raw blocks build_blocks makes from the entries."""
    import torch
    sets, _ = fixture
    dev = torch.device("cuda")
    for name, vi in (("fill256", 0), ("fill4096_internal", 1), ("varint", 1)):
        s = next(s for s in sets if s.name == name)
        v = s.variants[vi]
        with tab.open_table(v.file, internal_keys=bool(v.internal), resident=True) as t:
            r = t.scan_dev(max_blocks=4096)
            assert r["at_end"] and r["index_status"] == tab.LGS_ST_OK and r["n"] == len(s.entries)
            assert r["keys"].numel() >= r["key_bytes"] and r["key_bytes"] == sum(
                len(k) for k, _ in s.entries) + 16
            b = tab.build_blocks(r["keys"], r["key_off"], r["key_len"], r["vals"], r["val_off"],
                                 r["val_len"], v.block_size, v.restart_interval, bool(v.internal))
            torch.cuda.synchronize()
            with pytest.raises(Exception):
                tab.open_table(np.frombuffer(v.file, dtype=np.uint8).copy(),
                               internal_keys=bool(v.internal)).scan_dev()
        keys, koff, klen, vals, voff, vlen = tab._pack_entries(list(s.entries))

        def up(a, dt):
            return torch.from_numpy(a.view(dt).copy()).to(dev)

        w = tab.build_blocks(up(keys, np.uint8), up(koff, np.int64), up(klen, np.int32),
                             up(vals, np.uint8), up(voff, np.int64), up(vlen, np.int32),
                             v.block_size, v.restart_interval, bool(v.internal))
        torch.cuda.synchronize()
        assert b["nblocks"] == w["nblocks"] == len(v.blocks)
        assert bytes(b["raw"][:b["raw_total"]].cpu().numpy()) == bytes(
            w["raw"][:w["raw_total"]].cpu().numpy()) == b"".join(v.blocks)
        assert b["raw_len"].cpu().tolist() == w["raw_len"].cpu().tolist()
