"""tools/sim_compact_version.py (the CPU model of a compaction inside a
version) against what lcdb's own loop, its
ldb_compaction_should_stop_before and ldb_compaction_is_base_level_for_key
answered and wrote (tests/golden/compact_version.bin), and the model's parallel
formulation against its serial loop on seeded random cases."""
from __future__ import annotations

import hashlib
import os
import random
import sys

import pytest

import compact_version_golden_io as vio
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_compact_version as sim  # noqa: E402
import sim_merge  # noqa: E402
import sim_table_split  # noqa: E402
from sim_table_scan import ST_OK, Table, scan  # noqa: E402

CASES, COMPACT = vio.read()


def check_files(entries, first, images, files):
    assert len(images) == len(files)
    assert first == [sum(f.entries for f in files[:i]) for i in range(len(files) + 1)]
    for f, img, rec in zip(range(len(files)), images, files):
        assert (len(img), hashlib.sha256(img).digest()) == (rec.size, rec.sha256), f
        assert rec.image is None or rec.image == img, f
        assert (entries[first[f]][0], entries[first[f + 1] - 1][0]) == (rec.smallest, rec.largest)


def args_of(c):
    return (c.smallest_snapshot, c.levels, c.limit, c.block_size, c.restart_interval,
            c.compression, c.bits_per_key, c.max_output_file_size)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_serial_loop_is_lcdbs(case):
    keys = [k for k, _ in case.entries]
    stops, drops = sim.loop_serial(keys, case.smallest_snapshot, case.levels, case.limit)
    assert bytes(vio.STOP * s | vio.DROP * d for s, d in zip(stops, drops)) == case.flags
    kept, first, images = sim.compact_serial(case.entries, *args_of(case))
    assert kept == case.kept()
    check_files(kept, first, images, case.files)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_parallel_formulation_on_the_records(case):
    keys = [k for k, _ in case.entries]
    assert bytes(vio.STOP * s | vio.DROP * d for s, d in
                 zip(sim.stops_chain(keys, case.levels, case.limit),
                     sim.drop_flags(keys, case.smallest_snapshot, case.levels))) == case.flags
    kept, first, images = sim.compact_parallel(case.entries, *args_of(case))
    assert kept == case.kept()
    check_files(kept, first, images, case.files)


def merged_inputs(c):
    inputs = []
    for img in c.inputs:
        st, es = scan(Table(img, internal=True, filter_name=None))
        assert st == ST_OK
        inputs.append(es)
    return [inputs[r][i] for r, i in sim_merge.merge_serial(inputs, True)], inputs


def test_model_reproduces_the_compaction():
    c = COMPACT
    merged, inputs = merged_inputs(c)
    for route in (sim.compact_serial, sim.compact_parallel):
        kept, first, images = route(merged, *args_of(c))
        check_files(kept, first, images, c.files)
        assert all(f.image is not None for f in c.files)
    # The recorded compaction shows what it is there for.
    lv2 = c.levels[0]
    assert len(c.levels) == 1 and sum(s for _, _, s in lv2) > 10 << 20
    lo = min(es[0][0][:-8] for es in inputs)
    hi = max(es[-1][0][:-8] for es in inputs)
    assert lv2[0][1][:-8] < lo and lv2[-1][0][:-8] > hi          # files wholly before and behind
    assert len(c.files) >= 2 and c.files[0].size < c.max_output_file_size   # a stop closed it
    stops, drops = sim.loop_serial([k for k, _ in merged], c.smallest_snapshot, c.levels, c.limit)
    assert any(stops)
    covered = lambda u: any(a[:-8] <= u <= b[:-8] for a, b, _ in lv2)   # noqa: E731
    assert any(k[-8] == 0 and covered(k[:-8]) for k, _ in kept)
    assert any(d and k[-8] == 0 and not covered(k[:-8]) and
               (i == 0 or merged[i - 1][0][:-8] != k[:-8])
               for i, ((k, _), d) in enumerate(zip(merged, drops)))
    # Without the levels the files are not lcdb's: the feature is needed.
    plain, _, dropped = sim_merge.merge(inputs, True, True, c.smallest_snapshot, True)
    assert len(plain) != len(kept)


def test_whole_level_gives_the_overlapping_subsets_stops():
    """Level + 2 given whole yields what lcdb's c->grandparents, the files that
    overlap the inputs, yields: files before the inputs are passed by the first
    key at no cost, files behind them are never reached."""
    c = COMPACT
    merged, _ = merged_inputs(c)
    keys = [k for k, _ in merged]
    lo, hi = keys[0][:-8], keys[-1][:-8]
    subset = [f for f in c.levels[0] if f[1][:-8] >= lo and f[0][:-8] <= hi]
    assert 0 < len(subset) < len(c.levels[0]) - 1
    assert sim.stops_chain(keys, [subset], c.limit) == sim.stops_chain(keys, c.levels, c.limit) == \
        sim.loop_serial(keys, c.smallest_snapshot, [subset], c.limit)[0]


@pytest.mark.parametrize("seed", range(6))
def test_parallel_equals_serial_on_random_cases(seed):
    rng = random.Random(9000 + seed)
    stops_seen = forced_seen = 0
    for t in range(50):
        entries, snap, levels, limit = sim.random_case(rng)
        keys = [k for k, _ in entries]
        stops, drops = sim.loop_serial(keys, snap, levels, limit)
        assert sim.stops_chain(keys, levels, limit) == stops, t
        assert sim.drop_flags(keys, snap, levels) == drops, t
        args = (rng.choice([1, 64, 256]), rng.choice([1, 3, 16]), rng.choice([0, 1]),
                rng.choice([0, 10]), rng.choice([1, 100, 400, sim_table_split.NO_SPLIT]))
        want = sim.compact_serial(entries, snap, levels, limit, *args)
        assert sim.compact_parallel(entries, snap, levels, limit, *args) == want, t
        stops_seen += sum(stops)
        forced_seen += sum(sim.forced_flags(stops, drops))
    assert stops_seen >= forced_seen > 0            # a start needs a stop; the cases have both


def test_fixture_covers_the_edges():
    by = {c.name: c for c in CASES}
    assert sorted(len(by[f"files_{n}"].levels[0]) for n in (0, 1, 2, 65, 300)) == [0, 1, 2, 65, 300]
    assert sorted(len(by[f"entries_{n}"].entries) for n in (1, 2, 255, 256, 257, 5000)) == \
        [1, 2, 255, 256, 257, 5000]
    assert by["limit_zero"].limit == 0 and by["limit_exact"].limit == 1000
    c = by["stops_on_dropped"]
    assert sum(1 for f in c.flags if f == vio.STOP | vio.DROP) == 5 and len(c.files) == 3
    assert [f.entries for f in by["stop_behind_size_close"].files] == [1] * 9
    assert any(k[-8] > 1 for k, _ in by["odd_types"].entries)
    assert len(by["base_five_levels"].levels) == 5 and [] in by["base_five_levels"].levels
    assert by["forced_consecutive"].files[1].entries == 1
    assert by["forced_restart_1"].restart_interval == 1 and by["forced_snappy"].compression == 1
    assert by["forced_filter"].bits_per_key == 10 and len(by["forced_filter"].files) > 3
    assert by["forced_every_block_a_file"].max_output_file_size == 1
