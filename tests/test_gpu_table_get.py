"""Batched point lookups on the device: lgs_block_seek_dev and
lgs_table_get_host against what lcdb's own ldb_table_internal_get returned
(tests/golden/table_get.bin) and, for the larger shapes, against
tools/sim_table_get.py, which that fixture pins to the reference."""
from __future__ import annotations

import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

import damage_golden_io as dio
import table_get_golden_io as gio
import table_golden_io
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_table_get as sim  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_SEQ = (1 << 56) - 1


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


@pytest.fixture(scope="module")
def fixture():
    return table_golden_io.read(), gio.read()


def _check_case(tab, c, file):
    keys = [r.key for r in c.records]
    res, st, verdict = tab.get_host(file, keys, verify=bool(c.verify),
                                    paranoid_checks=bool(c.paranoid),
                                    internal_keys=bool(c.internal),
                                    filter_name=tab.FILTER_NAME if c.bits_per_key else None)
    for q, r in enumerate(c.records):
        what = (c.name, r.key[:40])
        assert table_io.same_outcome(int(st[q]), r.rc), (what, int(st[q]), r.rc)
        assert (res[q] is not None) == bool(r.called), what
        if r.called:
            assert res[q] == (r.found_key, r.found_value), what
        if c.internal:
            want = sim.verdict(r.found_key, r.key) if r.called else sim.NOTFOUND
            assert int(verdict[q]) == want, what


def _check_unopened(tab, c, file, keys):
    """A table lcdb did not open: its open status (under the INTEGRATION §3.1
    mapping) for every lookup, and nothing found."""
    fname = tab.FILTER_NAME if c.bits_per_key else None
    want = tab.index_host(file, paranoid_checks=bool(c.paranoid), internal_keys=bool(c.internal),
                          filter_name=fname)[3]
    assert table_io.same_outcome(want, c.open_rc), (c.name, want, c.open_rc)
    res, st, verdict = tab.get_host(file, keys, verify=bool(c.verify),
                                    paranoid_checks=bool(c.paranoid),
                                    internal_keys=bool(c.internal), filter_name=fname)
    assert res == [None] * len(keys) and list(st) == [want] * len(keys), c.name
    assert not verdict.any(), c.name


@pytest.mark.parametrize("group", ["bytewise", "internal", "patched", "damaged"])
def test_get_host_equals_the_reference(tab, fixture, group):
    """One lgs_table_get_host call per fixture table: called, status (under
    the INTEGRATION §3.1 mapping), key and value bytes as lcdb returned them;
    the verdict against save_value's rule on lcdb's recorded key.  "damaged":
    the randomly damaged tables of damage_get.bin, the ones lcdb did not open
    among them."""
    sets, cases = fixture
    n = 0
    for c in (dio.read_get() if group == "damaged" else cases):
        g = "patched" if c.patches else ("internal" if c.internal else "bytewise")
        if group != "damaged" and g != group:
            continue
        if group == "damaged" and c.open_rc != table_io.LDB_OK:
            s = next(s for s in sets if s.name == c.set_name)
            _check_unopened(tab, c, gio.table_of(c, sets), [k for k, _ in s.entries[:3]])
            n += 1
            continue
        assert c.open_rc == table_io.LDB_OK
        _check_case(tab, c, gio.table_of(c, sets))
        n += 1
    assert n >= 25


def _data_blocks(file: bytes):
    """The raw data blocks of an uncompressed table, through its index block."""
    t = sim.Table(file, filter_name=None)
    out = []
    for _, v in table_io.block_entries(t.index):
        h = sim.handle_import(v)
        if h is not None and h[0] + h[1] <= len(file):
            out.append(file[h[0]:h[0] + h[1]])
    return out


@pytest.mark.parametrize("internal", [0, 1])
def test_seek_blocks_equals_the_model(tab, fixture, internal):
    """lgs_block_seek_dev on the fixture's raw data blocks and on the patched
    tables' blocks: status, entry position, key and value as
    sim_table_get.block_seek has them."""
    sets, cases = fixture
    blocks, queries = [], []
    for c in cases:
        if c.internal != internal:
            continue
        if c.patches:
            if sets_variant(sets, c).compression:
                continue
            bl = _data_blocks(gio.table_of(c, sets))[:2]
        else:
            bl = sets_variant(sets, c).blocks
        keys = [r.key for r in c.records]
        keys = keys[::max(1, len(keys) * len(bl) // 96)]
        for b in bl:
            blocks.append(b)
            queries += [(len(blocks) - 1, k) for k in keys]
    if internal:
        # Versions of one user key in one block (tags inside the shared bytes).
        import sim_block_cut
        from test_table_get_sim import version_queries
        entries = gio.version_entries()
        for R in (16, 3, 1):
            blocks.append(sim_block_cut.serial_blocks(entries, 1 << 20, R)[1][0])
            queries += [(len(blocks) - 1, k) for k in version_queries(entries)]
    # Blocks too short to hold a restart count, and a block index out of range.
    for b in (b"", b"\0\0\0", b"\0\0\0\0", b"\1\0\0\0"):
        blocks.append(b)
        queries.append((len(blocks) - 1, b"abcdefgh1"))
    queries.append((0xFFFFFFFF, b"abcdefgh1"))
    assert len(blocks) > 100 and len(queries) > 3000
    res, st = tab.seek_blocks_host(blocks, queries, internal_keys=bool(internal))
    hits = 0
    for q, (b, k) in enumerate(queries):
        want_st, e = sim.block_seek(blocks[b], k, bool(internal)) if b < len(blocks) else (sim.ST_OK, None)
        assert int(st[q]) == want_st, (q, b, k[:40])
        if e is None:
            assert res[q] is None, (q, b, k[:40])
        else:
            blk = blocks[b]
            assert res[q] == (e[0], e[1], blk[e[2]:e[2] + e[3]]), (q, b, k[:40])
            hits += 1
    assert hits > 1000


@pytest.mark.parametrize("internal", [0, 1])
def test_seek_blocks_on_damaged_blocks(tab, fixture, internal):
    """lgs_block_seek_dev in one call on the randomly damaged data blocks of
    test_table_get_sim.damaged_blocks (over 400 for the two key kinds
    together, 6 to 10 targets each; the version blocks for internal keys) and
    on boundary_blocks' headers between decode_entry's two paths: status, entry position, key and value as sim_table_get.block_seek has
    them."""
    from test_table_get_sim import boundary_blocks, damaged_blocks
    sets, _ = fixture
    batch = damaged_blocks(sets, bool(internal))
    assert len(batch) >= 200
    batch += boundary_blocks(bool(internal))
    blocks = [d for d, _ in batch]
    queries = [(b, k) for b, (_, keys) in enumerate(batch) for k in keys]
    res, st = tab.seek_blocks_host(blocks, queries, internal_keys=bool(internal))
    hits = bad = 0
    for q, (b, k) in enumerate(queries):
        want_st, e = sim.block_seek(blocks[b], k, bool(internal))
        assert int(st[q]) == want_st, (q, b, k[:40])
        bad += want_st != sim.ST_OK
        if e is None:
            assert res[q] is None, (q, b, k[:40])
        else:
            blk = blocks[b]
            assert res[q] == (e[0], e[1], blk[e[2]:e[2] + e[3]]), (q, b, k[:40])
            hits += 1
    assert hits > 500 and bad > 50


def sets_variant(sets, c):
    return next(s for s in sets if s.name == c.set_name).variants[c.variant]


def test_block_status_makes_an_error_iterator(tab, fixture):
    sets, _ = fixture
    v = next(s for s in sets if s.name == "fill256").variants[0]
    b = v.blocks[0]
    k = table_io.block_entries(b)[0][0]
    res, st = tab.seek_blocks_host([b, b, b], [(0, k), (1, k), (2, k)],
                                   block_status=[tab.LGS_ST_OK, tab.LGS_ST_BADCRC, tab.LGS_ST_IOERR])
    assert res[0] is not None and res[1] is None and res[2] is None
    assert list(st) == [tab.LGS_ST_OK, tab.LGS_ST_BADCRC, tab.LGS_ST_IOERR]


def ik(user: bytes, seq: int, typ: int = 1) -> bytes:
    return user + struct.pack("<Q", (seq << 8) | typ)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """20 000 fillseq entries in 256-byte blocks with a bloom filter, written
    by lcdb (an index block over 64 KiB), and the model's view of it."""
    path = table_io.build_table(tmp_path_factory.mktemp("get"), 20000, 256, "cpu", 10)
    file = open(path, "rb").read()
    t = sim.Table(file, internal=True)
    assert t.status == sim.ST_OK and len(t.index) > 65536 and t.filter is not None
    return file, t


def _expect(tab, t, file, keys):
    res, st, verdict = tab.get_host(file, keys, verify=True, internal_keys=True)
    for q, k in enumerate(keys):
        called, wst, wk, wv = t.get(k, True)
        assert int(st[q]) == wst, (q, k)
        assert res[q] == ((wk, wv) if called else None), (q, k)
        assert int(verdict[q]) == (sim.verdict(wk, k) if called else sim.NOTFOUND), (q, k)
    return res


def test_large_table(tab, big):
    """20 000 lookups in one call: stored keys, misses, and 64 neighbouring
    keys 100 times over, so that each of their blocks (a 256-byte block holds
    two entries) is read once for 200 lookups."""
    file, t = big
    keys = [ik(b"%016d" % i, MAX_SEQ) for i in range(0, 20000, 2)]             # stored
    keys += [ik(b"%016d" % i, 0) for i in range(1, 3001, 3)]                   # older than stored
    keys += [ik(b"%016dx" % i, MAX_SEQ) for i in range(0, 20000, 10)]          # between two
    keys += [ik(b"%016d" % (20000 + i), MAX_SEQ) for i in range(600)]          # above the last
    keys += [ik(b"%016d" % (7000 + i), MAX_SEQ) for i in range(64)] * 100
    assert len(keys) == 20000
    res = _expect(tab, t, file, keys)
    assert sum(r is not None for r in res[:10000]) == 10000
    assert res[0][1] != res[1][1] and len(res[0][1]) == 100


@pytest.mark.parametrize("nq", [1, 63, 64, 65])
def test_query_counts_around_a_wave(tab, big, nq):
    file, t = big
    keys = [ik(b"%016d" % (311 * i % 20011), MAX_SEQ) for i in range(nq)]
    _expect(tab, t, file, keys)


def _raw_get(tab, file: bytes, keys, out_cap, null=None, nq=None):
    from lcdb_amd import _native
    L = _native.lib()
    img = np.frombuffer(file + b"\0", dtype=np.uint8)
    n = len(keys) if nq is None else nq
    kbuf, koff, klen = tab._pack_keys(keys)
    a = {"called": np.zeros(n + 1, dtype=np.uint8), "status": np.zeros(n + 1, dtype=np.uint8),
         "verdict": np.zeros(n + 1, dtype=np.uint8), "out": np.zeros(max(out_cap, 1), dtype=np.uint8),
         "koff": np.zeros(n + 1, dtype=np.uint64), "voff": np.zeros(n + 1, dtype=np.uint64)}
    need = C.c_size_t(12345)
    p = {k: (None if k == null else v.ctypes.data) for k, v in a.items()}
    rc = L.lgs_table_get_host(None if null == "file" else img.ctypes.data, len(file), 1, 0, 1,
                              tab.FILTER_NAME.encode(),
                              None if null == "keys" else kbuf.ctypes.data,
                              None if null == "key_off" else koff.ctypes.data,
                              None if null == "key_len" else klen.ctypes.data, n, p["called"],
                              p["status"], p["verdict"], p["out"], out_cap, p["koff"], p["voff"],
                              None if null == "needed" else C.byref(need))
    return rc, need.value, a


def test_arguments_and_out_cap(tab, big):
    from lcdb_amd import _native
    file, t = big
    keys = [ik(b"%016d" % i, MAX_SEQ) for i in (5, 77, 20001, 19999)]
    rc, need, a = _raw_get(tab, file, keys, 4096, nq=0)
    assert rc == _native.LGS_OK and need == 0 and a["koff"][0] == 0 and a["voff"][0] == 0
    for null in ("file", "keys", "key_off", "key_len", "called", "status", "out", "koff", "voff",
                 "needed"):
        assert _raw_get(tab, file, keys, 4096, null=null)[0] == _native.LGS_EINVAL, null
    assert _raw_get(tab, file, keys, 4096, null="verdict")[0] == _native.LGS_OK
    exact = 3 * (24 + 100)
    rc, need, a = _raw_get(tab, file, keys, exact - 1)
    assert rc == _native.LGS_ENOSPC and need == exact
    assert list(a["called"][:4]) == [1, 1, 0, 1]
    rc, need, a = _raw_get(tab, file, keys, exact)
    assert rc == _native.LGS_OK and need == exact
    assert int(a["koff"][4]) == exact and int(a["voff"][4]) == exact
    out = a["out"].tobytes()
    for q, i in ((0, 5), (1, 77), (3, 19999)):
        assert out[int(a["koff"][q]):int(a["voff"][q])] == ik(b"%016d" % i, i + 1)
        assert int(a["koff"][q + 1]) - int(a["voff"][q]) == 100
    assert int(a["koff"][2]) == int(a["voff"][2]) == int(a["koff"][3])
    # The Python wrapper's one retry with out_needed.
    res, st, _ = tab.get_host(file, keys, internal_keys=True, out_cap=1)
    assert [r is not None for r in res] == [True, True, False, True]


def test_tables_that_do_not_open(tab, big):
    file, _ = big
    keys = [ik(b"%016d" % 5, MAX_SEQ), ik(b"%016d" % 6, MAX_SEQ)]
    for bad in (file[:47], file[:-1] + bytes([file[-1] ^ 1])):
        want = tab.index_host(bad, internal_keys=True)[3]
        assert want == tab.LGS_ST_CORRUPT
        res, st, verdict = tab.get_host(bad, keys, internal_keys=True)
        assert res == [None, None] and list(st) == [want, want] and list(verdict) == [0, 0]
    # An index block that does not read: its read status, for every lookup.
    h = tab.index_host(file, paranoid_checks=True, internal_keys=True)
    assert h[3] == tab.LGS_ST_OK
    foot = file[-48:]
    at = 0
    for _ in range(2):
        _, at = table_io._varint(foot, at, 40, 64)
    ioff, _ = table_io._varint(foot, at, 40, 64)
    flip = bytearray(file)
    flip[ioff + 9] ^= 0x40
    want = tab.index_host(bytes(flip), paranoid_checks=True, internal_keys=True)[3]
    assert want == tab.LGS_ST_BADCRC
    res, st, _ = tab.get_host(bytes(flip), keys, paranoid_checks=True, internal_keys=True)
    assert res == [None, None] and list(st) == [want, want]
