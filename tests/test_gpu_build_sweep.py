"""The device table builder on the generated sweep:
build_blocks_host, build_table_host, build_tables_dev, build_blocks and
compact_to_files against what lcdb's own table builder wrote for every case
of tests/build_sweep.py (tests/golden/build_sweep.bin).  The fixture keeps
digests only; where a check needs bytes (the raw blocks, the index keys, the
first differing offset) they are the CPU model's, which reproduces every
recorded file (test_build_sweep_sim.py).  Every comparison is exact bytes."""
from __future__ import annotations

import hashlib
import random

import numpy as np
import pytest

import build_sweep as sweep
import build_sweep_golden_io as gio
from test_gpu_tables_build import images_of, upload

from sim_block_cut import index_keys, serial_blocks  # noqa: E402
import sim_merge  # noqa: E402
import sim_table_split as sim  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDS = gio.read()
NO_SPLIT = sweep.NO_SPLIT
SMALL = [r for r in RECORDS if not r.spec.startswith("large")]
LARGE = {r.spec: r for r in RECORDS if r.spec.startswith("large")}
CUTS = sorted({(r.spec, r.block_size, r.restart_interval, r.internal) for r in SMALL})


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


def sha(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def file_first(r):
    return [sum(f[0] for f in r.files[:i]) for i in range(len(r.files) + 1)]


def first_difference(got: bytes, want: bytes) -> str:
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} bytes, the model has {len(want)}; first difference at offset {at}"


def model_images(r):
    return sim.split_serial(sweep.entries(r.spec), r.block_size, r.restart_interval,
                            r.compression, r.bits_per_key, bool(r.internal), r.max_file_size)[1]


# ---- the cut, the raw blocks and the index keys ---------------------------------

@pytest.mark.parametrize("spec,block_size,R,internal", CUTS,
                         ids=[f"{s}/b{b}/r{R}" for s, b, R, _ in CUTS])
def test_blocks(tab, spec, block_size, R, internal):
    es = sweep.entries(spec)
    first, want = serial_blocks(es, block_size, R)
    blocks, got_first, ikeys = tab.build_blocks_host(es, block_size, R, bool(internal))
    assert got_first == first
    assert blocks == want
    assert ikeys == index_keys(es, first, bool(internal))


# ---- one file ---------------------------------------------------------------------

@pytest.mark.parametrize("r", [r for r in SMALL if r.max_file_size == NO_SPLIT],
                         ids=lambda r: r.name)
def test_table_host(tab, r):
    img = tab.build_table_host(sweep.entries(r.spec), r.block_size, r.restart_interval,
                               r.compression, r.bits_per_key, bool(r.internal))
    (rec,) = r.files
    if (len(img), sha(img)) != rec[1:]:
        pytest.fail(first_difference(img, model_images(r)[0]))


# ---- compaction's files -------------------------------------------------------------

def check_files(tab, r, b, scan=True):
    es = sweep.entries(r.spec)
    first, images = images_of(b)
    assert len(images) == len(r.files)
    assert first == file_first(r)
    for f, (img, rec) in enumerate(zip(images, r.files)):
        if (len(img), sha(img)) != rec[1:]:
            pytest.fail(f"file {f}: " + first_difference(img, model_images(r)[f]))
    if not scan:
        return
    for f, img in enumerate(images):
        with tab.open_table(img, internal_keys=bool(r.internal),
                            filter_name=tab.FILTER_NAME if r.bits_per_key else None) as t:
            assert list(t.scan()) == es[first[f]:first[f + 1]], f


def tables_dev(tab, run, r):
    return tab.build_tables_dev(run, r.block_size, r.restart_interval, r.compression,
                                r.bits_per_key, bool(r.internal), r.max_file_size)


@pytest.mark.parametrize("r", SMALL, ids=lambda r: r.name)
def test_tables_dev(tab, r):
    es = sweep.entries(r.spec)
    assert (len(es), gio.digest(es)) == (r.count, r.digest)
    check_files(tab, r, tables_dev(tab, upload(tab, es), r))


# ---- device input that is not packed --------------------------------------------------

def upload_loose(entries, shift: int):
    """upload()'s dict with the keys and values `shift` bytes into their buffers
    and 0-7 bytes of junk behind every entry: the offsets still increase."""
    import torch
    rng = random.Random(shift)
    run = {"n": len(entries)}
    for col, name in ((0, "key"), (1, "val")):
        buf, off = bytearray(b"\xa5" * shift), []
        for e in entries:
            off.append(len(buf))
            buf += e[col] + b"\x5a" * rng.randrange(8)
        off.append(len(buf))
        lens = np.array([len(e[col]) for e in entries], dtype=np.int32)
        assert any(off[i + 1] != off[i] + int(lens[i]) for i in range(len(entries)))
        run[name + "s"] = torch.from_numpy(np.frombuffer(bytes(buf) + b"\0" * 16,
                                                         dtype=np.uint8).copy()).cuda()
        run[name + "_off"] = torch.from_numpy(np.array(off, dtype=np.int64)).cuda()
        run[name + "_len"] = torch.from_numpy(lens).cuda()
        run[name + "_bytes"] = int(lens.sum())
    return run


LOOSE = [next(r for r in SMALL if r.spec.startswith(fam) and r.bits_per_key and r.compression
              and r.max_file_size not in (1, NO_SPLIT) and (r.internal or fam != "binary"))
         for fam in ("binary", "mixed", "jumbo")]


@pytest.mark.parametrize("shift", [1, 3, 13])
@pytest.mark.parametrize("r", LOOSE, ids=lambda r: r.name)
def test_device_input_that_is_not_packed(tab, r, shift):
    import torch
    es = sweep.entries(r.spec)
    run = upload_loose(es, shift)
    first, want = serial_blocks(es, r.block_size, r.restart_interval)
    b = tab.build_blocks(run["keys"], run["key_off"], run["key_len"], run["vals"], run["val_off"],
                         run["val_len"], r.block_size, r.restart_interval, bool(r.internal))
    torch.cuda.synchronize()
    raw, off, ln = (b[k].cpu().numpy() for k in ("raw", "raw_off", "raw_len"))
    assert b["nblocks"] == len(want)
    assert [int(x) for x in b["block_first"].cpu().numpy()] == first
    assert [raw[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln)] == want
    ik, io = b["ikey"].cpu().numpy(), b["ikey_off"].cpu().numpy()
    assert [ik[int(io[i]):int(io[i + 1])].tobytes() for i in range(len(want))] == \
        index_keys(es, first, bool(r.internal))
    check_files(tab, r, tables_dev(tab, run, r), scan=False)


# ---- generated compactions -------------------------------------------------------------

# (spec, runs, smallest_snapshot as a share of the highest sequence, drop_deletions,
#  max_output_file_size)
COMPACTIONS = [("binary:8:1", 3, 0.25, True, 1500), ("binary:8:1", 5, 0.6, False, 2500),
               ("random:115:513:1", 4, 0.5, True, 20000)]


@pytest.mark.parametrize("spec,nruns,share,drop_deletions,max_size", COMPACTIONS,
                         ids=[f"{c[0]}/{c[1]}runs/{'drop' if c[3] else 'keep'}" for c in COMPACTIONS])
def test_compact_to_files(tab, spec, nruns, share, drop_deletions, max_size):
    """Runs dealt from one internal set, so versions of a user key sit in
    different runs; deletions among them.  Inputs and expectation are the
    models' (sim_merge, sim_table_split), each pinned to lcdb by its fixture."""
    es = sweep.entries(spec)
    assert len(es) < 2000
    rng = random.Random(nruns)
    runs = [[] for _ in range(nruns)]
    for e in es:
        runs[rng.randrange(nruns)].append(e)
    users = [k[:-8] for k, _ in es]
    assert any(a == b for a, b in zip(users, users[1:])) and any(k[-8] == 0 for k, _ in es)
    where = {}
    for j, run in enumerate(runs):
        for k, _ in run:
            where.setdefault(k[:-8], set()).add(j)
    spread = sum(len(v) > 1 for v in where.values())
    assert spread >= 10
    snapshot = int(share * max(sim_merge.tag_of(k) >> 8 for k, _ in es))
    inputs = [sim.split_serial(run, 4096, 16, 0, 0, True)[1][0] for run in runs]
    kept, _, dropped = sim_merge.merge(runs, True, True, snapshot, drop_deletions)
    assert 0 < dropped < len(es)
    first, images = sim.split_serial(kept, 256, 7, 1, 10, True, max_size)
    assert len(images) > 2
    out = tab.compact_to_files(inputs, snapshot, drop_deletions, 256, 7, 1, 10,
                               max_output_file_size=max_size)
    assert len(out) == len(images)
    for f, (got, img) in enumerate(zip(out, images)):
        assert got["image"] == img, f"file {f}: " + first_difference(got["image"], img)
        assert (got["smallest"], got["largest"], got["entries"]) == \
            (kept[first[f]][0], kept[first[f + 1] - 1][0], first[f + 1] - first[f])


# ---- the kernels' own loops past their grid caps ------------------------------------------

@pytest.fixture(scope="module")
def large_model():
    """(digest of the concatenated blocks, block_first, index keys) of the
    large set's plain case, made once."""
    r = LARGE["large:0"]
    es = sweep.entries(r.spec)
    first, blocks = serial_blocks(es, r.block_size, r.restart_interval)
    return sha(b"".join(blocks)), first, index_keys(es, first, False)


def test_large_blocks(tab, large_model):
    """2^20 + 4099 entries: the second trip of emit_kernel's loop (more than
    65 536 workgroups of 16 entries) and of blocks_kernel's (more than 2048
    workgroups), and scan_top_kernel with two tile sums per thread."""
    r = LARGE["large:0"]
    es = sweep.entries(r.spec)
    assert len(es) == r.count > 65536 * 16 > 2048 * 256
    digest, first, ikeys = large_model
    blocks, got_first, got_ikeys = tab.build_blocks_host(es, r.block_size, r.restart_interval,
                                                         False)
    assert got_first == first
    assert sha(b"".join(blocks)) == digest
    assert got_ikeys == ikeys


def test_large_table_host(tab):
    r = LARGE["large:0"]
    img = tab.build_table_host(sweep.entries(r.spec), r.block_size, r.restart_interval,
                               r.compression, r.bits_per_key, False)
    assert [(r.count, len(img), sha(img))] == r.files


def test_large_tables_dev(tab):
    """The same counters under internal keys, snappy, a filter of 10 bits per
    key and files of 1 MiB: lcdb's per-file digests."""
    r = LARGE["large:1"]
    assert (r.compression, r.bits_per_key, r.max_file_size) == (1, 10, 1 << 20)
    b = tables_dev(tab, upload(tab, sweep.entries(r.spec)), r)
    first, images = images_of(b)
    assert first == file_first(r) and len(r.files) > 2
    assert [(len(i), sha(i)) for i in images] == [f[1:] for f in r.files]
