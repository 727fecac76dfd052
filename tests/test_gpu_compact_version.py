"""A compaction inside a version on the device:
lgs_merge_plan_version_dev / lgs_merge_stops_dev, lgs_block_cut_forced_dev,
lgs_tables_build_forced_dev, merge_runs_version, build_tables_dev(forced=...)
and compact_in_version against the files lcdb's own loop wrote with
ldb_compaction_should_stop_before and ldb_compaction_is_base_level_for_key at
work, and against one real lcdb compaction over a populated level 2
(tests/golden/compact_version.bin).  Every expectation is lcdb's record."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import pytest

import compact_version_golden_io as vio
import split_golden_io as sio
import table_golden_io
from merge_helpers import download, upload as upload_run
from test_gpu_tables_build import images_of, upload

pytestmark = pytest.mark.gpu

CASES, COMPACT = vio.read()
BY = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


def forced_of(case):
    """Per kept entry: lcdb closed the open output file just before it.  From
    the recorded files alone: a file start that no size-driven close explains
    is where a recorded stop (on that entry or on dropped ones before it) hit
    an open builder."""
    first = set(case.file_first()[1:-1])
    kept_at = [i for i, f in enumerate(case.flags) if not f & vio.DROP]
    out = []
    for k, p in enumerate(kept_at):
        lo = kept_at[k - 1] if k else -1
        out.append(int(k > 0 and any(case.flags[i] & vio.STOP for i in range(lo + 1, p + 1))))
    # Every forced start starts a recorded file, and where no size closes a
    # file they are all the starts there are.
    starts = {k for k, f in enumerate(out) if f}
    assert starts <= first, case.name
    assert case.max_output_file_size < 1 << 30 or starts == first, case.name
    return out


def merge_case(tab, case, runs=None):
    runs = [case.entries] if runs is None else runs
    return tab.merge_runs_version([upload_run(tab, r) for r in runs], case.smallest_snapshot,
                                  case.levels, case.limit)


def check_images(images, first, case):
    assert len(images) == len(case.files)
    assert first == case.file_first()
    for f, (img, rec) in enumerate(zip(images, case.files)):
        assert (len(img), hashlib.sha256(img).digest()) == (rec.size, rec.sha256), f
        assert rec.image is None or rec.image == img, f


# ---- the loop cases: plan, stops, forced build ----------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_loop_case_writes_lcdbs_files(tab, case):
    m = merge_case(tab, case)
    es, src = download(tab, m)
    kept = case.kept()
    assert es == kept                                              # lcdb's drops, entry for entry
    assert m["dropped"] == len(case.entries) - len(kept)
    want = forced_of(case)
    assert [int(x) for x in m["forced"].cpu().numpy()] == want
    assert m["n_forced"] == sum(want)
    b = tab.build_tables_dev(m, case.block_size, case.restart_interval, case.compression,
                             case.bits_per_key, True, case.max_output_file_size,
                             forced=m["forced"])
    first, images = images_of(b)
    check_images(images, first, case)
    if case.bits_per_key and len(images) > 1:
        # A later file's filter is over file-relative offsets: it opens and
        # finds its own keys.
        with tab.open_table(images[-1], internal_keys=True, filter_name=tab.FILTER_NAME) as t:
            assert list(t.scan()) == kept[first[-2]:]


@pytest.mark.parametrize("name", ["files_65", "odd_types", "entries_5000"])
def test_split_into_runs_gives_the_same_plan(tab, name):
    """The merged order is the merge's own when the entries come as 3 runs."""
    case = BY[name]
    runs = [case.entries[r::3] for r in range(3)]
    m = merge_case(tab, case, runs)
    es, _ = download(tab, m)
    assert es == case.kept()
    assert [int(x) for x in m["forced"].cpu().numpy()] == forced_of(case)


def test_no_levels_is_the_plain_plan(tab):
    """nlevels = 0: no stops, every key at base level: lgs_merge_plan_dev with
    drop_deletions = 1."""
    import torch
    case = BY["files_65"]
    runs = [upload_run(tab, case.entries[r::2]) for r in range(2)]
    v = tab.merge_runs_version(runs, case.smallest_snapshot, [], 0)
    p = tab.merge_runs(runs, internal_keys=True, drop=True,
                       smallest_snapshot=case.smallest_snapshot, drop_deletions=True)
    assert download(tab, v) == download(tab, p)
    assert (v["n"], v["dropped"], v["key_bytes"], v["val_bytes"], v["max_key"]) == \
        (p["n"], p["dropped"], p["key_bytes"], p["val_bytes"], p["max_key"])
    assert v["n_forced"] == 0 and not bool(torch.any(v["forced"] != 0))
    # And it differs from the plan with the levels: they matter.
    assert v["n"] != len(case.kept())


# ---- the forced cut by itself --------------------------------------------------

def cut(tab, run, case, forced):
    import torch
    from lcdb_amd import _native
    lib = _native.lib()
    n = run["n"]
    dev = run["keys"].device
    scr = torch.empty(int(lib.lgs_block_build_scratch(n)), dtype=torch.uint8, device=dev)
    bf = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    roff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rlen = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    ioff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    head = (run["keys"].data_ptr(), run["key_off"].data_ptr(), run["key_len"].data_ptr(),
            run["val_len"].data_ptr(), n, case.block_size, case.restart_interval, 1)
    tail = (bf.data_ptr(), roff.data_ptr(), rlen.data_ptr(), ioff.data_ptr(), counts.data_ptr(),
            scr.data_ptr(), int(scr.numel()), None)
    if forced is False:
        rc = lib.lgs_block_cut_dev(*head, *tail)
    else:
        rc = lib.lgs_block_cut_forced_dev(*head, None if forced is None else forced.data_ptr(),
                                          *tail)
    assert rc == _native.LGS_OK
    torch.cuda.synchronize()
    nb = int(counts[0])
    return [int(x) for x in bf[:nb + 1].cpu().numpy()], [int(x) for x in counts.cpu().numpy()]


@pytest.mark.parametrize("name", ["forced_at_block_start", "forced_before_block_start",
                                  "forced_behind_block_start", "forced_consecutive",
                                  "forced_restart_1"])
def test_forced_cut(tab, name):
    import torch
    case = BY[name]
    kept = case.kept()
    run = upload(tab, kept)
    want = forced_of(case)
    forced = torch.tensor(want, dtype=torch.int32, device="cuda")
    plain, plain_counts = cut(tab, run, case, False)
    assert cut(tab, run, case, None) == (plain, plain_counts)      # NULL: the existing call
    got, _ = cut(tab, run, case, forced)
    starts = [k for k, f in enumerate(want) if f]
    assert all(k in got for k in starts)
    # Up to the first forced start the size rule's blocks stand; a forced start
    # at a size-driven start changes nothing at all.
    assert [b for b in got if b <= starts[0]] == [b for b in plain if b < starts[0]] + [starts[0]]
    if name == "forced_at_block_start":
        assert got == plain
    if name == "forced_consecutive":
        assert starts[1] == starts[0] + 1                          # a block of one entry
    # The blocks are those of lcdb's files, each cut on its own.
    first = case.file_first()
    mine = []
    for f in range(len(first) - 1):
        sub, _ = cut(tab, upload(tab, kept[first[f]:first[f + 1]]), case, False)
        mine += [first[f] + b for b in sub[:-1]]
    assert got == mine + [len(kept)]


# ---- forced = None is the existing build -----------------------------------------

@pytest.mark.parametrize("name", ["gen300_1024_snappy", "gen300_internal_filter_snappy"])
def test_no_forced_flags_is_the_existing_build(tab, name):
    import torch
    case = next(c for c in sio.read()[0] if c.name == name)
    es = case.entries(table_golden_io.read())
    run = upload(tab, es)
    args = (case.block_size, case.restart_interval, case.compression, case.bits_per_key,
            bool(case.internal), case.max_file_size)
    old = images_of(tab.build_tables_dev(run, *args))
    assert [hashlib.sha256(i).digest() for i in old[1]] == [f.sha256 for f in case.files]
    zeros = torch.zeros(len(es), dtype=torch.int32, device="cuda")
    assert images_of(tab.build_tables_dev(run, *args, forced=zeros)) == old
    # The C call with NULL flags.
    rc, nf, used, b = call_forced(tab, run, case, None, case.max_file_size, 1 << 20, 64)
    from lcdb_amd import _native
    assert rc == _native.LGS_OK and images_of(b) == old


# ---- the real compaction, end to end -----------------------------------------------

def test_compact_in_version_writes_lcdbs_files(tab):
    c = COMPACT
    out = tab.compact_in_version(c.inputs, c.smallest_snapshot, c.levels, c.block_size,
                                 c.restart_interval, c.compression, c.bits_per_key,
                                 max_output_file_size=c.max_output_file_size)
    assert len(out) == len(c.files) >= 2
    for got, rec in zip(out, c.files):
        assert got["image"] == rec.image
        assert (got["smallest"], got["largest"], got["entries"]) == \
            (rec.smallest, rec.largest, rec.entries)
    # The limit given outright is the default's value.
    again = tab.compact_in_version(c.inputs, c.smallest_snapshot, c.levels, c.block_size,
                                   c.restart_interval, c.compression, c.bits_per_key,
                                   max_output_file_size=c.max_output_file_size,
                                   max_grandparent_overlap_bytes=c.limit)
    assert again == out
    # Without the levels it is another compaction: compact_to_files cannot write these.
    plain = tab.compact_to_files(c.inputs, c.smallest_snapshot, True, c.block_size,
                                 c.restart_interval, c.compression, c.bits_per_key,
                                 max_output_file_size=c.max_output_file_size)
    assert [f["image"] for f in plain] != [f.image for f in c.files]


# ---- errors ----------------------------------------------------------------------

def call_forced(tab, run, case, forced, max_file_size, files_cap, count_cap):
    """lgs_tables_build_forced_dev itself: (rc, n_files, files_bytes, outputs)."""
    import torch
    from lcdb_amd import _native
    dev = run["keys"].device
    files = torch.zeros(max(files_cap, 1) + 16, dtype=torch.uint8, device=dev)
    off = torch.zeros(max(count_cap, 1), dtype=torch.int64, device=dev)
    size = torch.zeros(max(count_cap, 1), dtype=torch.int64, device=dev)
    first = torch.zeros(max(count_cap, 1) + 1, dtype=torch.int32, device=dev)
    nf, used = C.c_uint32(77), C.c_uint64(77)
    rc = _native.lib().lgs_tables_build_forced_dev(
        *(run[f].data_ptr() for f in ("keys", "key_off", "key_len", "vals", "val_off", "val_len")),
        run["n"], run["key_bytes"], run["val_bytes"], case.block_size, case.restart_interval,
        case.compression, case.bits_per_key, getattr(case, "internal", 1), max_file_size,
        None if forced is None else forced.data_ptr(), files.data_ptr(), files_cap,
        off.data_ptr(), size.data_ptr(), first.data_ptr(), count_cap, C.byref(nf), C.byref(used),
        None)
    torch.cuda.synchronize()
    return rc, nf.value, used.value, {"files": files, "file_off": off[:nf.value],
                                      "file_size": size[:nf.value],
                                      "file_first": first[:nf.value + 1], "n_files": nf.value,
                                      "files_bytes": used.value}


def test_enospc_counts_the_forced_starts(tab):
    import torch
    from lcdb_amd import _native
    lib = _native.lib()
    case = BY["forced_consecutive"]
    kept = case.kept()
    run = upload(tab, kept)
    want = forced_of(case)
    forced = torch.tensor(want, dtype=torch.int32, device="cuda")
    files = len(case.files)
    assert files == 3 == 1 + sum(want)                             # all of them forced
    mx = case.max_output_file_size
    # The bound without the forced count is one file: too few.
    plain, bound = C.c_uint32(0), C.c_uint32(0)
    lib.lgs_tables_build_bound(run["n"], run["key_bytes"], run["val_bytes"], 0, mx, C.byref(plain))
    cap = lib.lgs_tables_build_forced_bound(run["n"], run["key_bytes"], run["val_bytes"], 0, mx,
                                            sum(want), C.byref(bound))
    assert plain.value == 1 and bound.value == 3
    rc, nf, need, b = call_forced(tab, run, case, forced, mx, 1 << 20, plain.value)
    assert (rc, nf) == (_native.LGS_ENOSPC, files) and 0 < need <= cap
    assert not b["file_off"].any() and not b["files"].any()
    rc, nf, used, b = call_forced(tab, run, case, forced, mx, need - 1, files)
    assert (rc, nf, used) == (_native.LGS_ENOSPC, files, need) and not b["files"].any()
    rc, nf, used, b = call_forced(tab, run, case, forced, mx, need, bound.value)
    assert (rc, nf, used) == (_native.LGS_OK, files, need)
    first, images = images_of(b)
    check_images(images, first, case)


def test_einval(tab):
    import torch
    from lcdb_amd import _native
    lib = _native.lib()
    case = BY["limit_exact"]
    run = upload_run(tab, case.entries)
    arr = (_native.LgsRun * 1)(_native.LgsRun(*(run[f].data_ptr() for f in
                                                 ("keys", "key_off", "key_len", "vals", "val_off",
                                                  "val_len")), run["n"]))
    counts = torch.full((8,), 77, dtype=torch.int64, device="cuda")

    def plan(levels, nlevels=None, scratch=None):
        lv, alive, nfiles, kb = tab._pack_levels(levels)
        size = int(lib.lgs_merge_version_scratch(run["n"], 1, nfiles, kb))
        scr = torch.empty(size if scratch is None else scratch, dtype=torch.uint8, device="cuda")
        rc = lib.lgs_merge_plan_version_dev(arr, 1, case.smallest_snapshot, lv,
                                            len(levels) if nlevels is None else nlevels,
                                            case.limit, counts.data_ptr(), scr.data_ptr(),
                                            int(scr.numel()), None)
        torch.cuda.synchronize()
        del alive
        return rc

    assert plan(case.levels) == _native.LGS_OK and int(counts[6]) == 2
    counts.fill_(77)
    short = [[(case.levels[0][0][0], b"1234567", 5)]]
    assert plan(short) == _native.LGS_EINVAL                       # a key under 8 bytes
    assert plan([[(b"abc", case.levels[0][0][1], 5)]]) == _native.LGS_EINVAL
    assert plan([[]] * 6) == _native.LGS_EINVAL                    # more than 5 levels
    assert plan(case.levels, scratch=64) == _native.LGS_EINVAL     # scratch too small
    assert plan([[]] * 5) == _native.LGS_OK
    assert [int(x) for x in counts.cpu().numpy()][6] == 0
    with pytest.raises(_native.LgsError):
        tab.merge_runs_version([run], 0, [[]] * 6, 0)
    # The flags come from the scratch of a plan over as many entries.
    forced = torch.zeros(4, dtype=torch.int32, device="cuda")
    scr = torch.zeros(int(lib.lgs_merge_version_scratch(4, 1, 0, 0)), dtype=torch.uint8, device="cuda")
    assert lib.lgs_merge_stops_dev(4, 5, forced.data_ptr(), scr.data_ptr(), int(scr.numel()),
                                   None) == _native.LGS_EINVAL
    assert lib.lgs_merge_stops_dev(4, 4, forced.data_ptr(), scr.data_ptr(), 8, None) == \
        _native.LGS_EINVAL
