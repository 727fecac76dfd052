"""The device compaction drop on the generated sweep:
merge_runs_host, merge_runs, compact_tables and compact_to_files against what
lcdb's own compaction loop kept and wrote for every case of
tests/merge_sweep.py (tests/golden/merge_sweep.bin), and, for the wide cases,
against the model's drop rule over the order lcdb's merging iterator
delivered.  test_merge_sweep_sim.py holds the model to the same records.
Every comparison is exact."""
from __future__ import annotations

import hashlib

import pytest

import merge_sweep as sweep
import merge_sweep_golden_io as gio
from merge_helpers import both

import sim_merge as sim  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDS = gio.read()
CASES = {c.name: c for c in sweep.all_cases()}
STEPS = [(s, runs) for r in RECORDS if r.kind == "repair"
         for s, runs in zip(r.steps, sweep.step_runs(CASES[r.name], r.steps))]
WIDE = [r for r in RECORDS if r.kind == "wide"]
STEP_IDS = [s.name for s, _ in STEPS]


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


@pytest.mark.parametrize("s,runs", STEPS, ids=STEP_IDS)
def test_recorded_steps(tab, s, runs):
    """What lcdb kept: the count, the digest, the entries where recorded; and
    the sources and the dropped count the model gives."""
    dd = bool(s.drop_deletions)
    got, src, dropped = both(tab, runs, internal_keys=True, drop=True,
                             smallest_snapshot=s.smallest_snapshot, drop_deletions=dd)
    want = sim.merge(runs, True, True, s.smallest_snapshot, dd)
    if got != want[0]:
        at = next((i for i, (a, b) in enumerate(zip(got, want[0])) if a != b),
                  min(len(got), len(want[0])))
        pytest.fail(f"{len(got)} entries kept, lcdb kept {s.count}; first difference at {at}: "
                    f"{got[at:at + 1]} for {want[0][at:at + 1]}")
    assert (len(got), gio.digest(got)) == (s.count, s.digest)
    if s.entries is not None:
        assert got == s.entries
    assert src == want[1] and dropped == want[2] == sum(len(r) for r in runs) - s.count


@pytest.mark.parametrize("s,runs", STEPS, ids=STEP_IDS)
def test_compaction_writes_the_recorded_file(tab, s, runs):
    """scan -> merge -> build over the input images, rebuilt from the
    regenerated entries: lcdb's output file byte for byte, or no file."""
    images = [tab.build_table_host(r, *sweep.OPTIONS, internal_keys=True) for r in runs]
    dd = bool(s.drop_deletions)
    files = tab.compact_to_files(images, s.smallest_snapshot, dd, *sweep.OPTIONS)
    if s.out_bytes is None:
        assert files == []
        return
    out = tab.compact_tables(images, s.smallest_snapshot, dd, *sweep.OPTIONS)
    assert (len(out), hashlib.sha256(out).digest()) == (s.out_bytes, s.out_sha256)
    kept = sim.merge(runs, True, True, s.smallest_snapshot, dd)[0]
    assert [(f["image"], f["smallest"], f["largest"], f["entries"]) for f in files] == \
        [(out, kept[0][0], kept[-1][0], s.count)]


@pytest.mark.parametrize("r", WIDE, ids=lambda r: r.name)
def test_wide_merges(tab, r):
    """k = 2 .. 64 tables: lcdb's merged order, then the model's drop rule over
    it at every snapshot of the case and both drop_deletions values."""
    c = CASES[r.name]
    runs = sweep.tables(c)
    got, src, dropped = both(tab, runs, internal_keys=True)
    assert dropped == 0 and (len(got), gio.digest(got)) == (r.count, r.digest)
    assert src == sim.merge(runs, True)[1]
    for snap in c.snapshots:
        for dd in (False, True):
            want = sim.merge(runs, True, True, snap, dd)
            got = both(tab, runs, internal_keys=True, drop=True, smallest_snapshot=snap,
                       drop_deletions=dd)
            assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (snap, dd)
