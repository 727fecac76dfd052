"""Opened-table handles on the device: lgs_table_open_host,
lgs_table_get, lgs_table_get_dev, lgs_table_info, lgs_table_close against what
lcdb's own ldb_table_internal_get returned (tests/golden/table_get.bin), against
tools/sim_table_get.py for the larger shapes, and against the unchanged
lgs_table_get_host."""
from __future__ import annotations

import bisect
import ctypes as C
import os
import struct
import sys
import threading

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
ALL_BLOCKS = 6667                  # data blocks of the `big` table


def ik(user: bytes, seq: int, typ: int = 1) -> bytes:
    return user + struct.pack("<Q", (seq << 8) | typ)


def stored(i: int) -> bytes:
    return ik(b"%016d" % i, MAX_SEQ)


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


@pytest.fixture(scope="module")
def native(gpu):
    from lcdb_amd import _native
    return _native


@pytest.fixture(scope="module")
def fixture():
    return table_golden_io.read(), gio.read()


class Big:
    """The `big` table of test_gpu_table_get.py and the model's answers on it,
    computed once per key and shared by every test here."""

    def __init__(self, file: bytes):
        self.file = file
        self.t = sim.Table(file, internal=True)
        self.seen = {}

    def want(self, k: bytes):
        r = self.seen.get(k)
        if r is None:
            r = self.seen[k] = self.t.get(k, True)
        return r


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    path = table_io.build_table(tmp_path_factory.mktemp("open"), 20000, 256, "cpu", 10)
    b = Big(open(path, "rb").read())
    assert b.t.status == sim.ST_OK and len(b.t.index) > 65536 and b.t.filter is not None
    return b


@pytest.fixture(scope="module")
def handles(tab, big):
    """One borrowed and one resident handle on `big`, open for the module."""
    img = np.frombuffer(big.file, dtype=np.uint8).copy()
    hs = {0: tab.open_table(img, internal_keys=True, resident=False),
          1: tab.open_table(big.file, internal_keys=True, resident=True)}
    assert hs[0].status == hs[1].status == tab.LGS_ST_OK
    yield hs
    for h in hs.values():
        h.close()


def _equals_model(big, keys, got):
    res, st, verdict = got
    assert len(res) == len(keys)
    for q, k in enumerate(keys):
        called, wst, wk, wv = big.want(k)
        assert int(st[q]) == wst, (q, k)
        assert res[q] == ((wk, wv) if called else None), (q, k)
        assert int(verdict[q]) == (sim.verdict(wk, k) if called else sim.NOTFOUND), (q, k)


def _group_of(c):
    return "patched" if c.patches else ("internal" if c.internal else "bytewise")


def _open_case(tab, c, file, resident):
    return tab.open_table(file if resident else np.frombuffer(file, dtype=np.uint8).copy(),
                          paranoid_checks=bool(c.paranoid), internal_keys=bool(c.internal),
                          filter_name=tab.FILTER_NAME if c.bits_per_key else None,
                          resident=bool(resident))


# ---- 1. reference parity -------------------------------------------------

def _cases_of(cases, group):
    """The fixture's cases of one group; "damaged": the randomly damaged tables
    of damage_get.bin, the ones lcdb did not open among them."""
    if group == "damaged":
        return dio.read_get()
    return [c for c in cases if _group_of(c) == group]


def _some_keys(sets, c):
    return [k for k, _ in next(s for s in sets if s.name == c.set_name).entries[:3]]


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("group", ["bytewise", "internal", "patched", "damaged"])
def test_get_equals_the_reference(tab, fixture, group, resident):
    """Every fixture case through one opened handle with one get: called,
    status (under the INTEGRATION §3.1 mapping), key and value bytes as lcdb
    returned them; the verdict against save_value's rule on lcdb's key.  A
    table lcdb did not open: its open status, and nothing found."""
    sets, cases = fixture
    n = 0
    for c in _cases_of(cases, group):
        if group == "damaged" and c.open_rc != table_io.LDB_OK:
            keys = _some_keys(sets, c)
            with _open_case(tab, c, gio.table_of(c, sets), resident) as t:
                assert table_io.same_outcome(t.status, c.open_rc), (c.name, t.status, c.open_rc)
                assert t.info()["status"] == t.status and t.info()["index_bytes"] == 0
                res, st, verdict = t.get(keys, verify=bool(c.verify))
                assert res == [None] * len(keys) and list(st) == [t.status] * len(keys), c.name
                assert not verdict.any(), c.name
            n += 1
            continue
        assert c.open_rc == table_io.LDB_OK
        with _open_case(tab, c, gio.table_of(c, sets), resident) as t:
            assert t.status == tab.LGS_ST_OK, c.name
            res, st, verdict = t.get([r.key for r in c.records], verify=bool(c.verify))
        for q, r in enumerate(c.records):
            what = (c.name, r.key[:40])
            assert table_io.same_outcome(int(st[q]), r.rc), (what, int(st[q]), r.rc)
            assert (res[q] is not None) == bool(r.called), what
            if r.called:
                assert res[q] == (r.found_key, r.found_value), what
            if c.internal:
                want = sim.verdict(r.found_key, r.key) if r.called else sim.NOTFOUND
                assert int(verdict[q]) == want, what
        n += 1
    assert n >= 25


# ---- 2. get_dev ----------------------------------------------------------

def _raw_get(native, t, keys, out_cap, null=None, nq=None, verify=1):
    """lgs_table_get with every array kept: (rc, out_needed, arrays)."""
    from lcdb_amd import table
    n = len(keys) if nq is None else nq
    kbuf, koff, klen = table._pack_keys(keys)
    a = {"called": np.zeros(n + 1, dtype=np.uint8), "status": np.zeros(n + 1, dtype=np.uint8),
         "verdict": np.zeros(n + 1, dtype=np.uint8), "out": np.zeros(max(out_cap, 1), dtype=np.uint8),
         "koff": np.full(n + 1, 77, dtype=np.uint64), "voff": np.full(n + 1, 77, dtype=np.uint64)}
    need = C.c_size_t(12345)
    p = {k: (None if k == null else v.ctypes.data) for k, v in a.items()}
    rc = native.lib().lgs_table_get(
        None if null == "table" else t._handle(), verify,
        None if null == "keys" else kbuf.ctypes.data,
        None if null == "key_off" else koff.ctypes.data,
        None if null == "key_len" else klen.ctypes.data, n, p["called"], p["status"],
        p["verdict"], p["out"], out_cap, p["koff"], p["voff"],
        None if null == "needed" else C.byref(need))
    return rc, need.value, a


def _dev_get(native, t, keys, out_cap, verify=1):
    """lgs_table_get_dev on uploaded keys, every output downloaded."""
    import torch
    from lcdb_amd import table
    n = len(keys)
    kbuf, koff, klen = table._pack_keys(keys)
    dev = torch.device("cuda")
    up = lambda a, dt: torch.from_numpy(a.view(dt).copy()).to(dev)   # noqa: E731
    d_k, d_koff, d_klen = up(kbuf, np.uint8), up(koff, np.int64), up(klen, np.int32)
    u8 = lambda m: torch.zeros(m, dtype=torch.uint8, device=dev)     # noqa: E731
    called, status, verdict, out = u8(n + 1), u8(n + 1), u8(n + 1), u8(max(out_cap, 1))
    okoff = torch.full((n + 1,), 77, dtype=torch.int64, device=dev)
    ovoff = torch.full((n + 1,), 77, dtype=torch.int64, device=dev)
    need = C.c_size_t(12345)
    rc = native.lib().lgs_table_get_dev(
        t._handle(), verify, d_k.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), n,
        called.data_ptr(), status.data_ptr(), verdict.data_ptr(), out.data_ptr(), out_cap,
        okoff.data_ptr(), ovoff.data_ptr(), C.byref(need), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    a = {"called": called.cpu().numpy(), "status": status.cpu().numpy(),
         "verdict": verdict.cpu().numpy(), "out": out.cpu().numpy(),
         "koff": okoff.cpu().numpy().view(np.uint64), "voff": ovoff.cpu().numpy().view(np.uint64)}
    return rc, need.value, a


def _same_arrays(a, b, n, total):
    for name in ("called", "status", "verdict"):
        assert a[name][:n].tobytes() == b[name][:n].tobytes(), name
    for name in ("koff", "voff"):
        assert a[name][:n + 1].tobytes() == b[name][:n + 1].tobytes(), name
    assert a["out"][:total].tobytes() == b["out"][:total].tobytes()


@pytest.mark.parametrize("group", ["bytewise", "internal", "patched", "damaged"])
def test_get_dev_equals_get(tab, native, fixture, group):
    """lgs_table_get_dev on a resident handle: every output, downloaded, is
    lgs_table_get's on the same handle byte for byte, out_key_off, out_val_off
    and out_needed included."""
    sets, cases = fixture
    n = 0
    for c in _cases_of(cases, group):
        keys = [r.key for r in c.records] or _some_keys(sets, c)
        cap = sum(len(r.found_key) + len(r.found_value) for r in c.records if r.called)
        with _open_case(tab, c, gio.table_of(c, sets), 1) as t:
            rc, need, a = _raw_get(native, t, keys, cap, verify=c.verify)
            rc2, need2, b = _dev_get(native, t, keys, cap, verify=c.verify)
        assert rc == rc2 == native.LGS_OK, c.name
        assert need == need2 == cap, c.name
        _same_arrays(a, b, len(keys), cap)
        n += 1
    assert n >= 25


def test_get_dev_through_the_wrapper(tab, big, handles):
    import torch
    keys = [stored(i) for i in (5, 77, 20001, 19999)]
    kbuf, koff, klen = tab._pack_keys(keys)
    up = lambda a, dt: torch.from_numpy(a.view(dt).copy()).cuda()    # noqa: E731
    r = handles[1].get_dev(up(kbuf, np.uint8), up(koff, np.int64), up(klen, np.int32), out_cap=1)
    torch.cuda.synchronize()
    assert r["out_needed"] == 3 * 124 and list(r["called"].cpu()) == [1, 1, 0, 1]
    out, ko, vo = r["out"].cpu().numpy(), r["out_key_off"].cpu().numpy(), r["out_val_off"].cpu().numpy()
    for q, k in enumerate(keys):
        called, _, wk, wv = big.want(k)
        assert out[ko[q]:vo[q]].tobytes() == wk and out[vo[q]:ko[q + 1]].tobytes() == wv


# ---- 3. reuse ------------------------------------------------------------

@pytest.mark.parametrize("resident", [0, 1])
def test_one_handle_many_gets(big, handles, resident):
    """Five gets in a row on one handle, each with other keys; query counts
    around a wave."""
    t = handles[resident]
    batches = [
        [stored(i) for i in range(0, 20000, 40)],                               # stored
        [ik(b"%016d" % i, 0) for i in range(1, 901, 3)]                         # older than stored
        + [ik(b"%016dx" % i, MAX_SEQ) for i in range(0, 20000, 100)],           # between two
        [stored(20000 + i) for i in range(300)],                                # above the last
        [stored(7000 + i) for i in range(64)] * 100,                            # 64 neighbours x 100
        [stored(i) for i in range(19999, 0, -57)],
    ]
    for keys in batches:
        _equals_model(big, keys, t.get(keys))
    for nq in (1, 63, 64, 65):
        keys = [stored(311 * i % 20011) for i in range(nq)]
        _equals_model(big, keys, t.get(keys))


# ---- 4. residency --------------------------------------------------------

def _index_and_filter_ranges(tab, file: bytes):
    foot = file[-48:]
    at = 0
    for _ in range(2):
        _, at = table_io._varint(foot, at, 40, 64)
    ioff, at = table_io._varint(foot, at, 40, 64)
    isize, _ = table_io._varint(foot, at, 40, 64)
    fh = tab.index_host(file, internal_keys=True)[2]
    assert fh is not None
    return (ioff, isize + 5), (fh[0], fh[1] + 5)


def test_the_blocks_stay_on_the_device(tab, big):
    """Nothing is read from the host's index and filter block after open (a
    borrowed image), nor from the host's image at all (a resident one)."""
    keys = [stored(i) for i in range(3, 20000, 173)] + [stored(20005)]
    keys += [ik(b"%016dx" % i, MAX_SEQ) for i in range(0, 2000, 50)]
    img = np.frombuffer(big.file, dtype=np.uint8).copy()
    with tab.open_table(img, internal_keys=True, resident=False) as t:
        for off, n in _index_and_filter_ranges(tab, big.file):
            img[off:off + n] = 0xFF
        _equals_model(big, keys, t.get(keys))
        info = t.info()
        assert info["status"] == tab.LGS_ST_OK and info["resident"] is False
        assert info["index_bytes"] == len(big.t.index)
        assert info["filter_bytes"] == len(big.t.filter)
        assert info["device_bytes"] >= len(big.t.index) + len(big.t.filter)
    img = np.frombuffer(big.file, dtype=np.uint8).copy()
    with tab.open_table(img, internal_keys=True, resident=True) as t:
        img[:] = 0
        _equals_model(big, keys, t.get(keys))
        info = t.info()
        assert info["resident"] is True and info["index_bytes"] == len(big.t.index)
        assert info["device_bytes"] >= len(big.file) + len(big.t.index)


# ---- 5. dedup shapes -----------------------------------------------------

@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("blocks", [1, 2047, 2048, 2049, ALL_BLOCKS])
def test_distinct_block_counts(big, handles, resident, blocks):
    """Queries that touch exactly `blocks` distinct blocks, up to every block
    of the table (the scan's part is 2 048 items; lcdb cuts this table into
    6 667 blocks of three entries, block b holding entries 3b .. 3b + 2)."""
    step = ALL_BLOCKS // blocks
    keys = [stored(3 * step * b) for b in range(blocks)]
    if blocks == 1:
        keys = [stored(4242), stored(4243)]
    # The index entry each key lands on: the first separator not below it (the
    # user keys differ, so their bytes decide).
    seps = [k[:-8] for k, _ in table_io.block_entries(big.t.index)]
    assert len(seps) == ALL_BLOCKS and seps == sorted(seps)
    assert len({bisect.bisect_left(seps, k[:-8]) for k in keys}) == blocks
    if blocks <= 2:
        assert sim.number_blocks(big.t, keys)[2] == blocks
    _equals_model(big, keys, handles[resident].get(keys))


@pytest.mark.parametrize("resident", [0, 1])
def test_dedup_edges(big, handles, resident):
    t = handles[resident]
    # 4 096 queries all in one block.
    keys = [stored(9000), stored(9001)] * 2048
    assert sim.number_blocks(big.t, keys[:2])[2] == 1
    _equals_model(big, keys, t.get(keys))
    # Every query a miss above the last key: the index seek finds no entry.
    keys = [stored(20000 + i) for i in range(130)]
    got = t.get(keys)
    assert got[0] == [None] * 130 and set(got[1]) == {sim.ST_OK}
    _equals_model(big, keys, got)
    # User keys the bloom filter rejects: no block is read at all.
    cand = [ik(b"%016dq" % i, MAX_SEQ) for i in range(0, 20000, 37)]
    keys = [k for k in cand if sim.index_lookup(big.t, k)[0] == 1 and not sim.index_lookup(big.t, k)[4]]
    assert len(keys) > 400 and sim.number_blocks(big.t, keys)[2] == 0
    res, st, verdict = t.get(keys)
    assert res == [None] * len(keys) and set(st) == {sim.ST_OK} and not verdict.any()
    # Descending key order: the numbering does not depend on the queries' order.
    keys = [stored(i) for i in range(19999, 0, -7)]
    _equals_model(big, keys, t.get(keys))


# ---- 6. arguments --------------------------------------------------------

def test_arguments_and_out_cap(tab, native, big, handles):
    L = native.lib()
    keys = [stored(i) for i in (5, 77, 20001, 19999)]
    for resident in (0, 1):
        t = handles[resident]
        rc, need, a = _raw_get(native, t, keys, 4096, nq=0)
        assert rc == native.LGS_OK and need == 0 and a["koff"][0] == 0 and a["voff"][0] == 0
        for null in ("table", "keys", "key_off", "key_len", "called", "status", "out", "koff",
                     "voff", "needed"):
            assert _raw_get(native, t, keys, 4096, null=null)[0] == native.LGS_EINVAL, null
        assert _raw_get(native, t, keys, 4096, null="verdict")[0] == native.LGS_OK
        exact = 3 * (24 + 100)
        rc, need, a = _raw_get(native, t, keys, exact - 1)
        assert rc == native.LGS_ENOSPC and need == exact
        assert list(a["called"][:4]) == [1, 1, 0, 1]
        assert list(a["status"][:4]) == [sim.ST_OK] * 4
        rc, need, a = _raw_get(native, t, keys, exact)
        assert rc == native.LGS_OK and need == exact
        assert int(a["koff"][4]) == exact and int(a["voff"][4]) == exact
        out = a["out"].tobytes()
        for q, i in ((0, 5), (1, 77), (3, 19999)):
            assert out[int(a["koff"][q]):int(a["voff"][q])] == ik(b"%016d" % i, i + 1)
            assert int(a["koff"][q + 1]) - int(a["voff"][q]) == 100
        assert int(a["koff"][2]) == int(a["voff"][2]) == int(a["koff"][3])
        # The Python wrapper's one retry with out_needed.
        res, st, _ = t.get(keys, out_cap=1)
        assert [r is not None for r in res] == [True, True, False, True]
    # get_dev: resident tables only; the same out_cap rule.
    assert _dev_get(native, handles[0], keys, 4096)[0] == native.LGS_EINVAL
    rc, need, a = _dev_get(native, handles[1], keys, exact - 1)
    assert rc == native.LGS_ENOSPC and need == exact and list(a["called"][:4]) == [1, 1, 0, 1]
    rc, need, a = _dev_get(native, handles[1], keys, exact)
    assert rc == native.LGS_OK and need == exact and int(a["koff"][4]) == exact
    # Open's own arguments; close(NULL).
    h, st = C.c_void_p(None), C.c_uint8(0)
    img = np.frombuffer(big.file, dtype=np.uint8)
    assert L.lgs_table_open_host(None, len(img), 0, 1, None, 0, C.byref(h), C.byref(st)) == native.LGS_EINVAL
    assert L.lgs_table_open_host(img.ctypes.data, len(img), 0, 1, None, 0, None, C.byref(st)) == native.LGS_EINVAL
    assert L.lgs_table_open_host(img.ctypes.data, len(img), 0, 1, None, 0, C.byref(h), None) == native.LGS_EINVAL
    assert L.lgs_table_open_host(img.ctypes.data, len(img), 0, 2, None, 0, C.byref(h), C.byref(st)) == native.LGS_EINVAL
    assert L.lgs_table_open_host(img.ctypes.data, len(img), 0, 1, None, 2, C.byref(h), C.byref(st)) == native.LGS_EINVAL
    assert L.lgs_table_info(None, None, None, None, None, None) == native.LGS_EINVAL
    L.lgs_table_close(None)


# ---- 7. tables that do not open ------------------------------------------

@pytest.mark.parametrize("resident", [0, 1])
def test_tables_that_do_not_open(tab, native, big, resident):
    file = big.file
    keys = [stored(5), stored(6)]
    foot = file[-48:]
    at = 0
    for _ in range(2):
        _, at = table_io._varint(foot, at, 40, 64)
    ioff, _ = table_io._varint(foot, at, 40, 64)
    flip = bytearray(file)
    flip[ioff + 9] ^= 0x40
    for bad, paranoid, want in ((file[:47], False, tab.LGS_ST_CORRUPT),
                                (file[:-1] + bytes([file[-1] ^ 1]), False, tab.LGS_ST_CORRUPT),
                                (bytes(flip), True, tab.LGS_ST_BADCRC)):
        assert tab.index_host(bad, paranoid_checks=paranoid, internal_keys=True)[3] == want
        t = tab.open_table(bad, paranoid_checks=paranoid, internal_keys=True, resident=bool(resident))
        assert t.status == want and t.info()["status"] == want
        assert t.info()["index_bytes"] == 0
        for _ in range(2):
            res, st, verdict = t.get(keys)
            assert res == [None, None] and list(st) == [want, want] and list(verdict) == [0, 0]
        rc, need, a = _raw_get(native, t, keys, 64)
        assert rc == native.LGS_OK and need == 0 and not a["koff"][:3].any() and not a["voff"][:3].any()
        if resident:
            rc, need, a = _dev_get(native, t, keys, 64)
            assert rc == native.LGS_OK and need == 0
            assert list(a["status"][:2]) == [want, want] and not a["called"][:2].any()
            assert not a["koff"][:3].any() and not a["voff"][:3].any() and not a["verdict"][:2].any()
        t.close()
        t.close()


# ---- 8. two threads, one handle ------------------------------------------

def test_two_threads_one_handle(tab, fixture, big, handles):
    """A handle is read-only after open: two threads, 20 gets of 500 keys each
    on one handle, while a second table is open beside it."""
    sets, cases = fixture
    c = next(c for c in cases if not c.patches and c.internal and c.bits_per_key)
    other_keys = [r.key for r in c.records]
    sets_keys = [[stored((7 * i + 13 * j) % 20400) for i in range(500)] for j in range(8)]
    for ks in sets_keys:
        for k in ks:
            big.want(k)
    errors = []

    def worker(t, first):
        try:
            for it in range(20):
                keys = sets_keys[(first + it) % 8]
                _equals_model(big, keys, t.get(keys))
        except BaseException as e:           # noqa: BLE001
            errors.append(e)

    with _open_case(tab, c, gio.table_of(c, sets), 1) as other:
        for resident in (0, 1):
            th = [threading.Thread(target=worker, args=(handles[resident], j)) for j in (0, 3)]
            for x in th:
                x.start()
            res, st, _ = other.get(other_keys, verify=bool(c.verify))
            for x in th:
                x.join()
            assert not errors, errors[0]
            for q, r in enumerate(c.records):
                assert (res[q] is not None) == bool(r.called)
                assert table_io.same_outcome(int(st[q]), r.rc)


# ---- 9. equivalence with the unchanged path ------------------------------

@pytest.mark.parametrize("resident", [0, 1])
def test_get_equals_get_host(tab, fixture, big, resident):
    sets, cases = fixture
    keys = [stored(i) for i in range(0, 20400, 29)] + [ik(b"%016dx" % i, MAX_SEQ) for i in range(0, 9000, 31)]
    want = tab.get_host(big.file, keys, internal_keys=True)
    with tab.open_table(big.file, internal_keys=True, resident=bool(resident)) as t:
        got = t.get(keys)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes()
    assert got[2].tobytes() == want[2].tobytes()
    picked = [next(c for c in cases if _group_of(c) == g and (g != "patched" or "handle_past" in c.name))
              for g in ("bytewise", "internal", "patched")]
    for c in picked:
        file = gio.table_of(c, sets)
        keys = [r.key for r in c.records]
        fname = tab.FILTER_NAME if c.bits_per_key else None
        want = tab.get_host(file, keys, verify=bool(c.verify), paranoid_checks=bool(c.paranoid),
                            internal_keys=bool(c.internal), filter_name=fname)
        with _open_case(tab, c, file, resident) as t:
            got = t.get(keys, verify=bool(c.verify))
        assert got[0] == want[0], c.name
        assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes(), c.name


# ---- 10. one handle, every kind of call in turn ---------------------------

def test_get_scan_and_get_host_interleaved_on_one_borrowed_handle(tab, fixture):
    """One borrowed handle serves a get, scans in windows of 2 blocks without
    and with a start key, and a get_host of the same keys beside it, in turn
    and twice over: each stages its block read in the leased context's pinned
    arena, and every result is what lcdb recorded for this table."""
    import sim_table_scan
    import table_scan_golden_io as sio
    sets, cases = fixture
    c = next(c for c in cases if c.name == "fill256_internal:1")
    sc = next(s for s in sio.read() if s.name == c.name)
    file = gio.table_of(c, sets)
    assert not c.patches and sio.table_of(sc, sets) == file and bool(sc.verify) == bool(c.verify)
    recs = c.records[::8]
    keys = [r.key for r in recs]
    assert 30 <= len(keys) <= 48 and any(r.called for r in recs) and not all(r.called for r in recs)
    runs = [next(r for r in sc.runs if r.start is None and r.count),
            next(r for r in sc.runs if r.start is not None and r.count)]

    def check_get(got):
        res, st, verdict = got
        for q, r in enumerate(recs):
            assert table_io.same_outcome(int(st[q]), r.rc), (q, int(st[q]), r.rc)
            assert res[q] == ((r.found_key, r.found_value) if r.called else None), q
            assert int(verdict[q]) == (sim.verdict(r.found_key, r.key) if r.called else sim.NOTFOUND), q

    def check_scan(t, r):
        ents = list(t.scan(start=r.start, verify=bool(c.verify), max_blocks=2))
        assert table_io.same_outcome(t.scan_status, r.rc)
        assert len(ents) == r.count and sim_table_scan.digest(ents) == r.digest
        assert r.entries is None or ents == r.entries

    fname = tab.FILTER_NAME if c.bits_per_key else None
    with _open_case(tab, c, file, 0) as t:
        assert t.status == tab.LGS_ST_OK
        for _ in range(2):
            check_get(t.get(keys, verify=bool(c.verify)))
            check_scan(t, runs[0])
            check_get(tab.get_host(file, keys, verify=bool(c.verify), paranoid_checks=bool(c.paranoid),
                                   internal_keys=bool(c.internal), filter_name=fname))
            check_scan(t, runs[1])
