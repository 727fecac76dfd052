"""The read side on the generated sweep: get_host,
OpenTable.get / get_dev, seek_blocks_host and OpenTable.scan(start=, end=)
against what lcdb's own ldb_table_internal_get and table iterator returned
for every target and scan start of tests/read_sweep.py
(tests/golden/read_sweep.bin).

The fixture keeps ordinals only.  A table's bytes are the CPU model's image,
used only where its length and SHA-256 are lcdb's; its entries are
regenerated, and test_read_sweep_sim.py holds their digests.  What stays the
model's: the raw data blocks and the index keys that seek_blocks_host is
given, and the offset of a found entry in its block.  Every comparison is
exact."""
from __future__ import annotations

import bisect
import functools

import numpy as np
import pytest

import read_sweep as rs
import read_sweep_golden_io as gio
import table_io

import sim_table_get as sim  # noqa: E402  (read_sweep put tools/ on the path)

pytestmark = pytest.mark.gpu

TABLES = rs.tables()
RECORDS = gio.read()
PAIRS = list(zip(TABLES, RECORDS))
IDS = [t.name for t in TABLES]
PLAIN = [(t, r) for t, r in PAIRS if not t.compression and not t.bits_per_key]
_IMAGES: dict = {}


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


def image(t, r) -> bytes:
    if t.name not in _IMAGES:
        _IMAGES[t.name] = rs.image(t, (r.size, r.sha) if t.versions else rs.sweep_pin(t))
    return _IMAGES[t.name]


def options(tab, t) -> dict:
    return {"internal_keys": bool(t.internal),
            "filter_name": tab.FILTER_NAME if t.bits_per_key else None}


def open_table(tab, t, r, resident):
    img = image(t, r)
    return tab.open_table(img if resident else np.frombuffer(img, dtype=np.uint8).copy(),
                          resident=bool(resident), **options(tab, t))


def lcdb_said(rc, fl, o) -> str:
    return f"lcdb: rc {rc}, called {fl & gio.CALLED}, entry {None if o == gio.NONE else o}"


def check_gets(t, r, how, res, st, verdict) -> None:
    """One batch of lookups against the record: status under same_outcome,
    called, the entry's bytes, and save_value's verdict on them."""
    es = rs.entries(t)
    for q, (k, rc, fl, o) in enumerate(zip(rs.targets(t), r.rc, r.flags, r.ordinal)):
        got = None if res[q] is None else (res[q][0][:40], res[q][1][:24])
        what = f"{t.name} {how}: target {k[:40]!r}; {lcdb_said(rc, fl, o)}; " \
               f"device: status {int(st[q])}, verdict {int(verdict[q])}, {got}"
        assert table_io.same_outcome(int(st[q]), rc), what
        assert (res[q] is not None) == bool(fl & gio.CALLED), what
        if fl & gio.CALLED:
            assert res[q] == es[o], what
        if t.internal:
            want = sim.verdict(es[o][0], k) if fl & gio.CALLED else sim.NOTFOUND
            assert int(verdict[q]) == want, what


@pytest.mark.parametrize("t,r", PAIRS, ids=IDS)
def test_get_host(tab, t, r):
    keys = rs.targets(t)
    for verify in (True, False) if not (t.compression or t.bits_per_key) else (True,):
        res, st, verdict = tab.get_host(image(t, r), keys, verify=verify, **options(tab, t))
        check_gets(t, r, f"get_host(verify={verify})", res, st, verdict)


@pytest.mark.parametrize("t,r", PAIRS, ids=IDS)
def test_open_table_get(tab, t, r):
    """OpenTable.get on a borrowed and on a resident image, and get_dev on
    device tensors equal to the resident get."""
    import torch
    keys = rs.targets(t)
    for resident in (0, 1):
        with open_table(tab, t, r, resident) as h:
            assert h.status == tab.LGS_ST_OK, t.name
            res, st, verdict = h.get(keys)
            check_gets(t, r, f"get(resident={resident})", res, st, verdict)
            if not resident:
                continue
            kbuf, koff, klen = tab._pack_keys(keys)
            up = lambda a, dt: torch.from_numpy(a.view(dt).copy()).cuda()   # noqa: E731
            d = h.get_dev(up(kbuf, np.uint8), up(koff, np.int64), up(klen, np.int32))
            torch.cuda.synchronize()
            called = d["called"].cpu().numpy()
            assert [bool(c) for c in called] == [x is not None for x in res], t.name
            assert d["status"].cpu().numpy().tobytes() == st.tobytes(), t.name
            assert d["verdict"].cpu().numpy().tobytes() == verdict.tobytes(), t.name
            out, ko, vo = (d[n].cpu().numpy() for n in ("out", "out_key_off", "out_val_off"))
            for q, x in enumerate(res):
                got = (out[ko[q]:vo[q]].tobytes(), out[vo[q]:ko[q + 1]].tobytes())
                assert got == (x if x is not None else (b"", b"")), (t.name, keys[q][:40], got)


@pytest.mark.parametrize("t,r", PLAIN, ids=[t.name for t, _ in PLAIN])
def test_seek_blocks_host(tab, t, r):
    """Every target against the raw block that lcdb's index names (the bisect
    of the index keys under the table's comparator; none past the last, and
    block 0 for a target too short to compare), all blocks in one call."""
    es = rs.entries(t)
    image(t, r)                                        # the SHA vouches for the model's cut
    _, blocks, ikeys = rs.cut(t)
    ck = functools.cmp_to_key(lambda a, b: sim.compare(a, b, bool(t.internal)))
    iks = [ck(k) for k in ikeys]
    keys = rs.targets(t)
    queries = []
    for k in keys:
        b = 0 if t.internal and len(k) < 8 else bisect.bisect_left(iks, ck(k))
        queries.append((b if b < len(blocks) else 0xFFFFFFFF, k))
    res, st = tab.seek_blocks_host(blocks, queries, internal_keys=bool(t.internal))
    for q, ((b, k), rc, fl, o) in enumerate(zip(queries, r.rc, r.flags, r.ordinal)):
        got = None if res[q] is None else (res[q][0], res[q][1][:40], res[q][2][:24])
        what = f"{t.name}: target {k[:40]!r} in block {b}; {lcdb_said(rc, fl, o)}; " \
               f"device: status {int(st[q])}, {got}"
        assert table_io.same_outcome(int(st[q]), rc), what
        if fl & gio.CALLED:
            at = sim.block_seek(blocks[b], k, bool(t.internal))[1][0]
            assert res[q] == (at,) + es[o], what
        else:
            assert res[q] is None, what


def scan(tab, h, **kw):
    """(final status, entries) of OpenTable.scan."""
    out = []
    try:
        for kv in h.scan(**kw):
            out.append(kv)
    except tab.ScanError as e:
        assert e.status == h.scan_status != tab.LGS_ST_OK
    return h.scan_status, out


# Windows of one block make a call per block, 4 101 of them in the largest
# table: there the starts go in two halves, a test each.
WINDOWS = [(t, r, w, half) for t, r in PAIRS for w in (1, 3, 4096)
           for half in ((0, 1) if w == 1 else (None,))]


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("t,r,width,half", WINDOWS,
                         ids=[f"{t.name}-w{w}" + ("" if h is None else "ab"[h])
                              for t, _, w, h in WINDOWS])
def test_scans_from_a_start(tab, t, r, width, half, resident):
    """scan(start=) in windows of 1, 3 and 4096 blocks: entries[ordinal:] and
    the recorded status."""
    es = rs.entries(t)
    runs = list(zip(rs.starts(t), r.starts))
    with open_table(tab, t, r, resident) as h:
        assert h.status == tab.LGS_ST_OK, t.name
        for s, (rc, count, o) in runs if half is None else runs[half::2]:
            st, got = scan(tab, h, start=s, max_blocks=width)
            what = f"{t.name}: start {s[:40]!r}, windows of {width}; lcdb: rc {rc}, {count} " \
                   f"entries from {o}; device: status {st}, {len(got)} entries" + \
                   (f" from {got[0][0][:40]!r}" if got else "")
            assert table_io.same_outcome(st, rc), what
            assert got == es[o:], what


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("t,r", PAIRS, ids=IDS)
def test_end_cuts(tab, t, r, resident):
    """scan(start=s, end=e) for the ordered pairs of the first six starts:
    lcdb's own seek to e is where the cut lies, no model between."""
    es = rs.entries(t)
    six = [(s, x[2]) for s, x in list(zip(rs.starts(t), r.starts))[:6] if x[0] == table_io.LDB_OK]
    with open_table(tab, t, r, resident) as h:
        assert h.status == tab.LGS_ST_OK, t.name
        for s, os_ in six:
            for e, oe in six:
                if e == s:
                    continue
                st, got = scan(tab, h, start=s, end=e)
                what = f"{t.name}: start {s[:40]!r}, end {e[:40]!r}; lcdb: entries {os_} to " \
                       f"{max(os_, oe)}; device: status {st}, {len(got)} entries"
                assert st == tab.LGS_ST_OK and got == es[os_:max(os_, oe)], what
