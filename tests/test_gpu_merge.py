"""Merging sorted runs on the device: lgs_merge_host and
lgs_merge_plan_dev / _emit_dev against what lcdb's own merging iterator
delivered and its own compactions wrote (tests/golden/merge.bin), and against
tools/sim_merge.py, which tests/test_merge_sim.py holds to the same fixture."""
from __future__ import annotations

import hashlib
import os
import sys
import threading

import pytest

import merge_golden_io as mio
import table_golden_io
import table_io
from merge_helpers import binary_users, both, download, ikey, on_device, run_of, upload

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_merge as sim  # noqa: E402

pytestmark = pytest.mark.gpu

MERGES, STEPS = mio.read()


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


@pytest.fixture(scope="module")
def sets():
    return table_golden_io.read()


@pytest.mark.parametrize("case", MERGES, ids=lambda c: c.name)
def test_fixture_merges(tab, sets, case):
    runs = [r.entries(sets) for r in case.runs]
    got, src, dropped = both(tab, runs, internal_keys=bool(case.internal))
    assert dropped == 0 and len(got) == case.count
    assert mio.digest(got) == case.digest
    if case.entries is not None:
        assert got == case.entries
    assert src == sim.merge(runs, bool(case.internal))[1]


@pytest.mark.parametrize("step", STEPS, ids=lambda s: s.name)
def test_fixture_compactions(tab, step):
    runs = [es for _, es in step.inputs]
    got, src, dropped = both(tab, runs, internal_keys=True, drop=True,
                             smallest_snapshot=step.smallest_snapshot,
                             drop_deletions=bool(step.drop_deletions))
    assert got == step.out_entries
    assert dropped == sum(len(r) for r in runs) - len(step.out_entries)
    assert [runs[r][i] for r, i in src] == got


@pytest.mark.parametrize("step", STEPS, ids=lambda s: s.name)
def test_compact_tables_writes_the_reference_file(tab, step):
    out = tab.compact_tables([img for img, _ in step.inputs], step.smallest_snapshot,
                             bool(step.drop_deletions), block_size=step.block_size,
                             restart_interval=step.restart_interval,
                             compression=step.compression, bits_per_key=step.bits_per_key)
    assert len(out) == step.out_bytes
    assert hashlib.sha256(out).digest() == step.out_sha256


def deal(n: int, k: int, internal: bool, dup: int = 3):
    """n entries over k runs: keys with `dup` copies each (ties across runs),
    dealt so that run sizes differ, each run sorted."""
    es = []
    for i in range(n):
        u = b"k%06d" % (i // dup)
        es.append((ikey(u, 7 + i % 2, i % 2) if internal else u, b"%d" % i))
    runs = [[] for _ in range(k)]
    for i, e in enumerate(es):
        runs[(i * 7 + i // 5) % k].append(e)
    return [sorted(r, key=sim.sort_key(internal)) for r in runs]


@pytest.mark.parametrize("internal", [False, True], ids=["bytewise", "internal"])
@pytest.mark.parametrize("k,n", [(0, 0), (1, 0), (1, 63), (2, 64), (3, 65), (5, 257), (64, 4097),
                                 (7, 4097)])
def test_shapes_against_the_model(tab, k, n, internal):
    runs = deal(n, k, internal) if k else []
    if k == 2:
        runs = [deal(n, 1, internal)[0], []]           # one run of two empty
    want = sim.merge(runs, internal)
    got = both(tab, runs, internal_keys=internal)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == 0
    if internal:
        for snap, dd in ((0, False), (7, True), (7, False), (8, True)):
            want = sim.merge(runs, True, True, snap, dd)
            got = both(tab, runs, internal_keys=True, drop=True, smallest_snapshot=snap,
                       drop_deletions=dd)
            assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]


def test_all_entries_equal(tab):
    for internal in (False, True):
        k = ikey(b"same", 4) if internal else b"same"
        runs = [[(k, b"r%dn%d" % (r, i)) for i in range(40 + r)] for r in range(5)]
        want = sim.merge(runs, internal)
        got = both(tab, runs, internal_keys=internal)
        assert got[0] == want[0] and got[1] == want[1]
        assert got[1] == [(r, i) for r in range(5) for i in range(40 + r)]


def test_keys_sharing_a_16_byte_prefix(tab):
    p = b"0123456789abcdef"
    for internal in (False, True):
        ks = [p + bytes([i % 5]) * (i % 4) + b"%03d" % (i % 50) for i in range(300)]
        es = [((ikey(k, 1 + i % 3) if internal else k), b"%d" % i) for i, k in enumerate(ks)]
        runs = [sorted(es[r::4], key=sim.sort_key(internal)) for r in range(4)]
        want = sim.merge(runs, internal)
        got = both(tab, runs, internal_keys=internal)
        assert got[0] == want[0] and got[1] == want[1]


@pytest.mark.parametrize("k", [2, 3, 5])
def test_binary_keys(tab, k):
    """About 600 distinct keys of \\0, \\xff and `a` bytes around the 8-byte
    word, dealt over k runs of unequal size with equal user keys in different
    runs: entries, sources and dropped counts equal the model's, plain and
    with the compaction drop at every snapshot."""
    import random
    rng = random.Random(600 + k)
    # Bytewise: every third key also in the next run (ties across runs).
    runs = [[] for _ in range(k)]
    for i, u in enumerate(binary_users(rng, 600)):
        r = run_of(i, k)
        runs[r].append((u, b"%d" % i))
        if i % 3 == 0:
            runs[(r + 1) % k].append((u, b"dup%d" % i))
    runs = [sorted(r, key=sim.sort_key(False)) for r in runs]
    assert len({len(r) for r in runs}) == k
    want = sim.merge(runs, False)
    got = both(tab, runs, internal_keys=False)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == 0
    # Internal: versions (seq 0..3, type 0 / 1) of one user key in different runs.
    runs = [[] for _ in range(k)]
    n = 0
    for i, u in enumerate(binary_users(rng, 220)):
        r = run_of(i, k)
        for j, seq in enumerate(rng.sample(range(4), rng.randint(1, 4))):
            runs[(r + j) % k].append((ikey(u, seq, rng.randrange(2)), b"%d.%d" % (i, seq)))
            n += 1
    runs = [sorted(r, key=sim.sort_key(True)) for r in runs]
    assert 500 <= n <= 700 and len({len(r) for r in runs}) == k
    want = sim.merge(runs, True)
    got = both(tab, runs, internal_keys=True)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == 0
    for snap in (0, 1, 2, 3):
        for dd in (False, True):
            want = sim.merge(runs, True, True, snap, dd)
            got = both(tab, runs, internal_keys=True, drop=True, smallest_snapshot=snap,
                       drop_deletions=dd)
            assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (snap, dd)


def test_one_entry_against_five_thousand(tab):
    big = [(b"key%08d" % (2 * i), b"") for i in range(5000)]
    for one in (b"key%08d" % 4999, b"key%08d" % 5000, b"", b"zzz"):
        for runs in ([[(one, b"x")], big], [big, [(one, b"x")]]):
            want = sim.merge(runs)
            got = both(tab, runs)
            assert got[0] == want[0] and got[1] == want[1]


def test_too_many_runs(tab):
    from lcdb_amd import _native
    runs = [[(b"k%02d" % r, b"")] for r in range(65)]
    with pytest.raises(tab.MergeError) as e:
        tab.merge_runs_host(runs)
    assert e.value.rc == _native.LGS_EINVAL and e.value.untouched
    with pytest.raises(_native.LgsError, match=r"\(-1\)"):
        tab.merge_runs([upload(tab, r) for r in runs])
    assert _native.lib().lgs_merge_scratch(10, 65) == 0


def test_unsorted_run_is_refused(tab):
    from lcdb_amd import _native
    good = [(b"a", b"1"), (b"c", b"2")]
    bad = [(b"b", b"3"), (b"a", b"4")]
    with pytest.raises(tab.MergeError) as e:
        tab.merge_runs_host([good, good, bad, bad])
    assert e.value.rc == _native.LGS_EINVAL and e.value.untouched
    with pytest.raises(tab.MergeError) as e:
        tab.merge_runs([upload(tab, r) for r in (good, good, bad, bad)])
    assert e.value.rc == _native.LGS_EINVAL and e.value.run == 2
    # Internal keys: sorted by raw bytes is not sorted, and a short key.
    a, b = ikey(b"ab", 5), ikey(b"ab\x01", 1)
    assert a > b
    with pytest.raises(tab.MergeError) as e:
        tab.merge_runs_host([[(b, b""), (a, b"")]], internal_keys=True)
    assert e.value.rc == _native.LGS_EINVAL
    assert tab.merge_runs_host([[(a, b""), (b, b"")]], internal_keys=True)[1] == [(0, 0), (0, 1)]
    with pytest.raises(tab.MergeError) as e:
        tab.merge_runs_host([[(a, b"")], [(b"short", b"")]], internal_keys=True)
    assert e.value.rc == _native.LGS_EINVAL and e.value.untouched
    with pytest.raises(tab.MergeError):
        tab.merge_runs_host([good], drop=True)         # drop needs internal keys


def test_host_capacities_too_small(tab):
    from lcdb_amd import _native
    runs = deal(100, 3, False)
    want = sim.merge(runs)
    n, kb, vb = len(want[0]), sum(len(k) for k, _ in want[0]), sum(len(v) for _, v in want[0])
    for caps in ((n - 1, kb, vb), (n, kb - 1, vb), (n, kb, vb - 1), (0, 0, 0)):
        with pytest.raises(tab.MergeError) as e:
            tab.merge_runs_host(runs, caps=caps)
        assert e.value.rc == _native.LGS_ENOSPC and e.value.untouched
        assert e.value.needed == (n, kb, vb, max(len(k) for k, _ in want[0]), 0)
    assert tab.merge_runs_host(runs, caps=(n, kb, vb))[0] == want[0]


def test_scan_merge_build_without_a_download(tab, sets):
    """scan_dev -> merge_runs -> build_blocks on device tensors equals the
    host route over the same entries."""
    s = next(x for x in sets if x.name == "fill4096_internal")
    v = next(v for v in s.variants if v.compression == 0)
    halves = [s.entries[0::2], s.entries[1::2]]
    images = [tab.build_table_host(h, internal_keys=True, compression=0) for h in halves]
    assert tab.build_table_host(s.entries, internal_keys=True, compression=0) == v.file
    opened = [tab.open_table(img, internal_keys=True, resident=True, filter_name=None)
              for img in images]
    try:
        runs = [t.scan_dev() for t in opened]
        assert all(r["at_end"] for r in runs)
        m = tab.merge_runs(runs, internal_keys=True)
        b = tab.build_blocks(m["keys"], m["key_off"], m["key_len"], m["vals"], m["val_off"],
                             m["val_len"], internal_keys=True)
        raw = b["raw"].cpu().numpy()
        off, ln = b["raw_off"].cpu().numpy(), b["raw_len"].cpu().numpy()
        blocks = [raw[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(b["nblocks"])]
    finally:
        for t in opened:
            t.close()
    want_entries = sim.merge(halves, True)[0]
    assert want_entries == s.entries
    assert blocks == tab.build_blocks_host(want_entries, internal_keys=True)[0] == v.blocks


def test_two_threads_on_their_own_streams(tab):
    import torch
    jobs = [(deal(3000, 5, True), dict(internal_keys=True, drop=True, smallest_snapshot=7,
                                       drop_deletions=True)),
            (deal(2500, 9, False), dict())]
    single = [on_device(tab, runs, **kw) for runs, kw in jobs]
    up = [[upload(tab, r) for r in runs] for runs, _ in jobs]
    torch.cuda.synchronize()
    out, errs = [None, None], []

    def work(j):
        try:
            st = torch.cuda.Stream()
            for _ in range(3):
                with torch.cuda.stream(st):
                    m = tab.merge_runs(up[j], stream=st, **jobs[j][1])
                st.synchronize()
                es, src = download(tab, m)
                out[j] = (es, src, m["dropped"])
        except Exception as e:                         # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for j in range(2):
        assert out[j][0] == single[j][0] and out[j][1] == single[j][1] and \
            out[j][2] == single[j][2]
