"""Compaction's output tables built on the device:
lgs_tables_build_dev, build_tables_dev, compact_to_files and compact_tables
against the files lcdb's own table builder and one of its own compactions
wrote (tests/golden/compact_split.bin, table_build.bin, merge.bin)."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import pytest

import merge_golden_io as mio
import split_golden_io as sio
import table_golden_io

pytestmark = pytest.mark.gpu

CASES, COMPACT = sio.read()
SETS = table_golden_io.read()
NO_SPLIT = sio.NO_SPLIT


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


def upload(tab, entries):
    """Entries as device tensors: the dict merge_runs returns."""
    import torch
    dev = torch.device("cuda")
    keys, koff, klen, vals, voff, vlen = tab._pack_entries(entries)
    koff = np.append(koff, np.uint64(klen.sum()))
    voff = np.append(voff, np.uint64(vlen.sum()))

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)

    return {"keys": up(keys, np.uint8), "key_off": up(koff, np.int64),
            "key_len": up(klen, np.int32), "vals": up(vals, np.uint8),
            "val_off": up(voff, np.int64), "val_len": up(vlen, np.int32), "n": len(entries),
            "key_bytes": int(klen.sum()), "val_bytes": int(vlen.sum())}


def images_of(b):
    """([file_first], [image bytes]) of a build_tables_dev result."""
    files = b["files"].cpu().numpy()
    off, size = b["file_off"].cpu().numpy(), b["file_size"].cpu().numpy()
    assert len(off) == len(size) == b["n_files"] and all(int(o) % 16 == 0 for o in off)
    assert all(int(off[f]) + int(size[f]) <= int(off[f + 1]) for f in range(len(off) - 1))
    assert b["n_files"] == 0 or int(off[-1]) + int(size[-1]) <= b["files_bytes"]
    return ([int(x) for x in b["file_first"].cpu().numpy()],
            [files[int(o):int(o) + int(s)].tobytes() for o, s in zip(off, size)])


def build(tab, entries, v, max_file_size, stream=None):
    return tab.build_tables_dev(upload(tab, entries), v.block_size, v.restart_interval,
                                v.compression, v.bits_per_key, bool(v.internal), max_file_size,
                                stream=stream)


# ---- one file: build_table_host's image ---------------------------------------

@pytest.mark.parametrize("s", [s for s in SETS if s.entries], ids=lambda s: s.name)
def test_one_file_is_the_host_build(tab, s):
    for v in s.variants:
        first, images = images_of(build(tab, s.entries, v, NO_SPLIT))
        assert first == [0, len(s.entries)]
        assert images == [v.file]                   # what lcdb wrote
        assert images[0] == tab.build_table_host(s.entries, v.block_size, v.restart_interval,
                                                 v.compression, v.bits_per_key, bool(v.internal))


def test_no_entries_no_file(tab):
    import torch
    z8 = torch.zeros(16, dtype=torch.uint8, device="cuda")
    z64 = torch.zeros(1, dtype=torch.int64, device="cuda")
    z32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    run = {"keys": z8, "key_off": z64, "key_len": z32[:0], "vals": z8, "val_off": z64,
           "val_len": z32[:0], "n": 0, "key_bytes": 0, "val_bytes": 0}
    b = tab.build_tables_dev(run, bits_per_key=10, internal_keys=True, max_file_size=1024)
    assert b["n_files"] == 0 and b["files_bytes"] == 0 and images_of(b) == ([0], [])


# ---- the fixture's splits -------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_fixture_splits(tab, case):
    es = case.entries(SETS)
    assert (len(es), sio.digest(es)) == (case.count, case.digest)
    first, images = images_of(build(tab, es, case, case.max_file_size))
    assert len(images) == len(case.files)
    assert first == [sum(f.entries for f in case.files[:i]) for i in range(len(case.files) + 1)]
    for f, (img, rec) in enumerate(zip(images, case.files)):
        assert (len(img), hashlib.sha256(img).digest()) == (rec.size, rec.sha256), f
        assert rec.image is None or rec.image == img, f
    # Round trip: every image opens and scans back to its entries.
    for f, img in enumerate(images):
        with tab.open_table(img, internal_keys=bool(case.internal),
                            filter_name=tab.FILTER_NAME if case.bits_per_key else None) as t:
            assert list(t.scan()) == es[first[f]:first[f + 1]], f


def test_index_key_cases_are_in_the_fixture():
    by = {c.name: c for c in CASES}
    assert by["gen300_filter"].bits_per_key == 10 and \
        all(f.size > 3 * 2048 for f in by["gen300_filter"].files[:-1])
    ff = by["last_user_key_all_ff"]
    assert ff.internal and ff.files[-1].largest[:-8] == b"\xff" * 6 and len(ff.files) > 1
    assert by["successors_internal_every_entry"].max_file_size == 1
    assert by["gen300_every_block"].max_file_size == 1
    assert by["gen300_exact_plus_1"].max_file_size == by["gen300_exact"].max_file_size + 1


# ---- a real compaction ----------------------------------------------------------

@pytest.fixture(scope="module")
def compaction_inputs(tab):
    c = COMPACT
    inputs, last = sio.compact_inputs(c.l0_files, c.user_keys)
    assert last == c.smallest_snapshot
    images = []
    for es, (n, sha) in zip(inputs, c.inputs):
        img = tab.build_table_host(es, c.block_size, c.restart_interval, c.compression,
                                   c.bits_per_key, internal_keys=True)
        assert len(es) == n and hashlib.sha256(img).digest() == sha
        images.append(img)
    return list(reversed(images))                   # newest level-0 file first


def test_compact_to_files_writes_lcdbs_files(tab, compaction_inputs):
    c = COMPACT
    out = tab.compact_to_files(compaction_inputs, c.smallest_snapshot, bool(c.drop_deletions),
                               c.block_size, c.restart_interval, c.compression, c.bits_per_key,
                               max_output_file_size=c.max_file_size)
    assert len(out) == len(c.files) == 3
    for got, rec in zip(out, c.files):
        assert (len(got["image"]), hashlib.sha256(got["image"]).digest()) == (rec.size, rec.sha256)
        assert (got["smallest"], got["largest"], got["entries"]) == \
            (rec.smallest, rec.largest, rec.entries)


@pytest.mark.parametrize("step", mio.read()[1], ids=lambda s: s.name)
def test_compact_tables_still_writes_the_reference_file(tab, step):
    out = tab.compact_tables([img for img, _ in step.inputs], step.smallest_snapshot,
                             bool(step.drop_deletions), block_size=step.block_size,
                             restart_interval=step.restart_interval,
                             compression=step.compression, bits_per_key=step.bits_per_key)
    assert (len(out), hashlib.sha256(out).digest()) == (step.out_bytes, step.out_sha256)


# ---- errors -----------------------------------------------------------------------

def call(tab, run, case, max_file_size, files_cap, count_cap):
    """lgs_tables_build_dev itself: (rc, n_files, files_bytes, outputs)."""
    import torch
    from lcdb_amd import _native
    dev = run["keys"].device
    files = torch.zeros(max(files_cap, 1) + 16, dtype=torch.uint8, device=dev)
    off = torch.zeros(max(count_cap, 1), dtype=torch.int64, device=dev)
    size = torch.zeros(max(count_cap, 1), dtype=torch.int64, device=dev)
    first = torch.zeros(max(count_cap, 1) + 1, dtype=torch.int32, device=dev)
    nf, used = C.c_uint32(77), C.c_uint64(77)
    rc = _native.lib().lgs_tables_build_dev(
        *(run[f].data_ptr() for f in ("keys", "key_off", "key_len", "vals", "val_off", "val_len")),
        run["n"], run["key_bytes"], run["val_bytes"], case.block_size, case.restart_interval,
        case.compression, case.bits_per_key, case.internal, max_file_size, files.data_ptr(),
        files_cap, off.data_ptr(), size.data_ptr(), first.data_ptr(), count_cap, C.byref(nf),
        C.byref(used), None)
    torch.cuda.synchronize()
    return rc, nf.value, used.value, {"files": files, "file_off": off[:nf.value],
                                      "file_size": size[:nf.value],
                                      "file_first": first[:nf.value + 1], "n_files": nf.value,
                                      "files_bytes": used.value}


def test_errors(tab):
    from lcdb_amd import _native
    case = next(c for c in CASES if c.name == "gen300_1024")
    es = case.entries(SETS)
    run = upload(tab, es)
    want = len(case.files)
    rc, nf, used, _ = call(tab, run, case, 0, 1 << 20, 64)
    assert (rc, nf, used) == (_native.LGS_EINVAL, 0, 0)
    rc, nf, need, b = call(tab, run, case, 1024, 1 << 20, want - 1)
    assert (rc, nf) == (_native.LGS_ENOSPC, want) and 0 < need < (1 << 20)
    assert not b["file_off"].any() and not b["files"].any()
    rc, nf, used, b = call(tab, run, case, 1024, need - 1, want)
    assert (rc, nf, used) == (_native.LGS_ENOSPC, want, need)
    assert not b["files"].any()
    rc, nf, used, b = call(tab, run, case, 1024, need, want)
    assert (rc, nf, used) == (_native.LGS_OK, want, need)
    first, images = images_of(b)
    assert [hashlib.sha256(i).digest() for i in images] == [f.sha256 for f in case.files]
    cap = _native.lib().lgs_tables_build_bound(run["n"], run["key_bytes"], run["val_bytes"],
                                               0, 1024, None)
    assert need <= cap


# ---- a side stream ------------------------------------------------------------------

def test_side_stream(tab):
    import torch
    case = next(c for c in CASES if c.name == "gen300_internal_filter_snappy")
    es = case.entries(SETS)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        run = upload(tab, es)                       # produced on the stream that builds
        b = tab.build_tables_dev(run, case.block_size, case.restart_interval, case.compression,
                                 case.bits_per_key, True, case.max_file_size, stream=stream)
    stream.synchronize()
    first, images = images_of(b)
    assert [hashlib.sha256(i).digest() for i in images] == [f.sha256 for f in case.files]
    assert first[-1] == len(es)
