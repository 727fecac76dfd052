"""The device data-block builder and the one-call table build:
lgs_block_* and lgs_table_build_host against tables written by lcdb's own
ldb_tablegen_* -- the committed fixture (tests/golden/table_build.bin) and
build_table.cpu's files.  Every comparison is exact bytes."""
from __future__ import annotations

import os
import struct
import sys

import numpy as np
import pytest

import table_golden_io
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_block_cut as sim  # noqa: E402

pytestmark = pytest.mark.gpu

SETS = table_golden_io.read()
REF_TABLES = [(20000, 4096, 0), (1500, 256, 10), (12000, 65536, 0)]


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


_ref_cache: dict = {}


@pytest.fixture(scope="module")
def ref_table(tmp_path_factory):
    """(file bytes, its data blocks, their handles, entries) of a build_table.cpu
    table, made once."""
    def get(entries: int, block_size: int, bloom: int):
        key = (entries, block_size, bloom)
        if key not in _ref_cache:
            tmp = tmp_path_factory.mktemp("ref")
            path = table_io.build_table(tmp, entries, block_size, "cpu", bloom)
            d = table_io.dump_blocks(path, str(tmp / "dump.bin"), verify=True)
            assert all(rc == table_io.LDB_OK for rc in d.rc)
            data = d.contents[:-2]              # then the metaindex and index blocks
            ents = [e for c in data for e in table_io.block_entries(c)]
            assert len(ents) == entries
            handles = (d.off[:-2], d.size[:-2])
            _ref_cache[key] = (open(path, "rb").read(), data, handles, ents)
        return _ref_cache[key]
    return get


# ---- 1. fixture cases -------------------------------------------------------

@pytest.mark.parametrize("s", SETS, ids=[s.name for s in SETS])
def test_fixture_tables(tab, s):
    assert s.variants
    for v in s.variants:
        what = (s.name, v.block_size, v.restart_interval, v.compression, v.bits_per_key)
        got = tab.build_table_host(s.entries, v.block_size, v.restart_interval, v.compression,
                                   v.bits_per_key, bool(v.internal))
        assert got == v.file, what
        blocks, first, ikeys = tab.build_blocks_host(s.entries, v.block_size, v.restart_interval,
                                                     bool(v.internal))
        assert blocks == v.blocks, what
        assert ikeys == v.ikeys, what
        assert first[0] == 0 and first[-1] == len(s.entries) and len(first) == len(v.blocks) + 1


# ---- 2. the reference's whole write path ------------------------------------

@pytest.mark.parametrize("entries,block_size,bloom", REF_TABLES)
def test_reference_tables(tab, ref_table, entries, block_size, bloom):
    want, _, _, ents = ref_table(entries, block_size, bloom)
    got = tab.build_table_host(ents, block_size, 16, tab.LGS_SNAPPY_COMPRESSION, bloom, True)
    assert len(got) == len(want)
    assert got == want


def test_reference_table_with_index_block_over_64k(tab, ref_table):
    """6 667 data blocks: an index block of several 64 KiB encoder chunks
    (the table tail encodes them as separate items), and a filter block."""
    want, data, _, ents = ref_table(20000, 256, 10)
    assert len(data) > 6000
    handles, _, _, st = tab.index_host(want, internal_keys=True)
    assert st == tab.LGS_ST_OK and len(handles) == len(data)
    got = tab.build_table_host(ents, 256, 16, tab.LGS_SNAPPY_COMPRESSION, 10, True)
    assert got == want
    got0 = tab.build_table_host(ents, 256, 16, tab.LGS_NO_COMPRESSION, 10, True)
    foot = got0[-48:]
    vals, at = [], 0
    for _ in range(4):
        v, at = table_io._varint(foot, at, 40, 64)
        vals.append(v)
    assert vals[3] > 3 * 65536                    # the raw index block
    assert [e for h in tab.index_host(got0, internal_keys=True)[0]
            for e in table_io.block_entries(got0[h[0]:h[0] + h[1]])] == ents


# ---- 3. device-resident -----------------------------------------------------

def _device_entries(torch, ents, shift: int):
    """Keys and values packed at `shift` bytes into their buffers."""
    out = []
    for col in (0, 1):
        lens = np.array([len(e[col]) for e in ents], dtype=np.int32)
        off = np.zeros(len(ents), dtype=np.int64)
        off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        buf = np.frombuffer(b"\xa5" * shift + b"".join(e[col] for e in ents) + b"\0" * 16,
                            dtype=np.uint8)
        out += [torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(off + shift).cuda(),
                torch.from_numpy(lens).cuda()]
    return out


def _check_device_result(r, data):
    raw = r["raw"].cpu().numpy()
    off, ln = r["raw_off"].cpu().numpy(), r["raw_len"].cpu().numpy()
    nb = len(data)
    assert r["nblocks"] == nb
    got = [raw[int(off[b]):int(off[b]) + int(ln[b])].tobytes() for b in range(nb)]
    assert got == data
    assert int(off[nb]) == r["raw_total"] == sum(len(c) for c in data)
    assert r["max_len"] == max(len(c) for c in data)
    first = r["block_first"].cpu().numpy()
    counts = np.cumsum([0] + [len(table_io.block_entries(c)) for c in data])
    assert [int(x) for x in first] == [int(x) for x in counts]


@pytest.mark.parametrize("shift,side_stream", [(0, False), (0, True), (1, False), (3, False),
                                               (13, False)])
def test_build_blocks_on_device(tab, ref_table, shift, side_stream):
    import torch
    file, data, (h_off, h_size), ents = ref_table(20000, 4096, 0)
    args = _device_entries(torch, ents, shift)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side_stream else None
    r = tab.build_blocks(*args, block_size=4096, restart_interval=16, internal_keys=True,
                         stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    _check_device_result(r, data)
    # The index keys are the keys of the reference's index block.
    _, keys, _, st = tab.index_host(file, internal_keys=True)
    assert st == tab.LGS_ST_OK
    ik, io = r["ikey"].cpu().numpy(), r["ikey_off"].cpu().numpy()
    assert [ik[int(io[b]):int(io[b + 1])].tobytes() for b in range(len(data))] == keys
    # The result is write_blocks' input as it stands.
    _, hoff, hsize, end = tab.write_blocks(r["raw"], r["raw_off"], r["raw_len"],
                                           max_len=r["max_len"], raw_total=r["raw_total"])
    torch.cuda.synchronize()
    assert [int(x) for x in hoff.cpu()] == [int(x) for x in h_off]
    assert [int(x) for x in hsize.cpu()] == [int(x) for x in h_size]


# ---- 4. a deep chain ----------------------------------------------------------

@pytest.mark.parametrize("block_size", [1, 4096])
def test_deep_chain(tab, block_size):
    """70 000 blocks of one entry: 17 doubling rounds, multi-workgroup scans."""
    ents = [(struct.pack(">Q", 3 * i + 1), struct.pack("<I", i * 2654435761 & 0xffffffff))
            for i in range(70000)]
    first, want = sim.serial_blocks(ents, block_size, 16)
    blocks, got_first, ikeys = tab.build_blocks_host(ents, block_size, 16, False)
    assert len(blocks) == len(want) and (block_size != 1 or len(want) == 70000)
    assert got_first == first
    assert blocks == want
    assert ikeys == sim.index_keys(ents, first, False)


# ---- 5. the reference reader accepts the result -------------------------------

def _largest_fixture():
    s, v = max(((s, v) for s in SETS for v in s.variants), key=lambda p: len(p[1].file))
    return s.entries, v.block_size, v.restart_interval, v.compression, v.bits_per_key, bool(v.internal)


@pytest.mark.parametrize("which", ["fixture", "fillseq1500"])
def test_reference_reader_accepts(tab, ref_table, tmp_path, which):
    if which == "fixture":
        ents, bs, R, comp, bpk, internal = _largest_fixture()
    else:
        ents, bs, R, comp, bpk, internal = ref_table(1500, 256, 10)[3], 256, 16, 1, 10, True
    img = tab.build_table_host(ents, bs, R, comp, bpk, internal)
    path = tmp_path / "000001.ldb"
    path.write_bytes(img)
    d = table_io.dump_blocks(str(path), str(tmp_path / "dump.bin"), verify=True)
    assert d.file_size == len(img)
    assert all(rc == table_io.LDB_OK for rc in d.rc)
    handles, _, fh, st = tab.index_host(img, paranoid_checks=True, internal_keys=internal)
    assert st == tab.LGS_ST_OK and d.n - 2 == len(handles) > 0   # + metaindex and index
    assert (fh is not None) == (bpk > 0)
    assert [e for c in d.contents[:-2] for e in table_io.block_entries(c)] == ents


# ---- 6. argument errors ---------------------------------------------------------

def test_argument_errors(tab):
    from lcdb_amd._native import LgsError
    ok = [(b"k%07d" % i, b"v") for i in range(4)]
    assert len(tab.build_table_host(ok)) > 74
    with pytest.raises(LgsError, match=r"\(-5\)"):          # LGS_ENOSPC
        tab.build_table_host(ok, file_cap=16)
    with pytest.raises(LgsError, match=r"\(-5\)"):          # known only after the build
        tab.build_table_host(ok, file_cap=100)
    with pytest.raises(LgsError, match=r"\(-1\)"):          # LGS_EINVAL: a 7-byte internal key
        tab.build_table_host([(b"1234567", b"v")], internal_keys=True)
    with pytest.raises(LgsError, match=r"\(-1\)"):
        tab.build_blocks_host([(b"1234567", b"v")], internal_keys=True)
    with pytest.raises(LgsError, match=r"\(-1\)"):
        tab.build_table_host(ok, restart_interval=0)
    # An entry of 2^30 bytes: the lengths alone decide, no byte of it is read.
    import ctypes as C
    L = tab._L
    klen = np.array([8], dtype=np.uint32)
    vlen = np.array([(1 << 30) - 8], dtype=np.uint32)
    zero = np.zeros(1, dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint8)
    size = C.c_size_t(0)
    rc = L.lgs_table_build_host(buf.ctypes.data, zero.ctypes.data, klen.ctypes.data,
                                buf.ctypes.data, zero.ctypes.data, vlen.ctypes.data, 1, 4096, 16,
                                1, 0, 0, buf.ctypes.data, 64, C.byref(size))
    assert rc == -1
