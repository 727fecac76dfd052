"""tools/sim_table_split.py (the CPU model of compaction's output files,
DESIGN §4.9) against what lcdb's own table builder and one of its own
compactions wrote (tests/golden/compact_split.bin)."""
from __future__ import annotations

import hashlib
import os
import sys

import pytest

import split_golden_io as sio
import table_golden_io
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_merge  # noqa: E402
import sim_table_split as sim  # noqa: E402

CASES, COMPACT = sio.read()


@pytest.fixture(scope="module")
def sets():
    return table_golden_io.read()


def check_files(entries, first, images, files):
    assert len(images) == len(files)
    assert first == [sum(f.entries for f in files[:i]) for i in range(len(files) + 1)]
    for f, img, rec in zip(range(len(files)), images, files):
        assert (len(img), hashlib.sha256(img).digest()) == (rec.size, rec.sha256), f
        assert rec.image is None or rec.image == img, f
        assert (entries[first[f]][0], entries[first[f + 1] - 1][0]) == (rec.smallest, rec.largest)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_model_reproduces_every_split_record(case, sets):
    es = case.entries(sets)
    assert (len(es), sio.digest(es)) == (case.count, case.digest)
    first, images = sim.split_serial(es, case.block_size, case.restart_interval, case.compression,
                                     case.bits_per_key, bool(case.internal), case.max_file_size)
    check_files(es, first, images, case.files)
    assert sim.split_blocks(es, case.block_size, case.restart_interval, case.compression,
                            case.max_file_size) == first


def test_model_reproduces_the_compaction():
    c = COMPACT
    inputs, last = sio.compact_inputs(c.l0_files, c.user_keys)
    assert last == c.smallest_snapshot and [len(es) for es in inputs] == [n for n, _ in c.inputs]
    kept, _, _ = sim_merge.merge(list(reversed(inputs)), True, True, c.smallest_snapshot,
                                 bool(c.drop_deletions))
    first, images = sim.split_serial(kept, c.block_size, c.restart_interval, c.compression,
                                     c.bits_per_key, True, c.max_file_size)
    assert len(images) == 3
    check_files(kept, first, images, c.files)


def test_fixture_covers_the_edges():
    by = {c.name: c for c in CASES}
    every = by["gen300_every_block"]
    assert every.max_file_size == 1 and len(every.files) > 40
    a, b = by["gen300_exact"], by["gen300_exact_plus_1"]
    assert b.max_file_size == a.max_file_size + 1 and a.files[0].entries < b.files[0].entries
    assert len(by["gen300_one_file"].files) == 1
    assert any(c.bits_per_key and any(f.size > 3 * 2048 for f in c.files) for c in CASES)
    ff = by["last_user_key_all_ff"]
    assert ff.internal and ff.files[-1].largest[:-8] == b"\xff" * 6
