"""tools/sim_block_cut.py (no GPU): its serial restatement of lcdb's block cut
is pinned to the reference, and the parallel formulation lgs_block.hip runs
 equals the serial one."""
from __future__ import annotations

import os
import random
import sys

import pytest

import table_golden_io
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_block_cut as sim  # noqa: E402


@pytest.mark.parametrize("block_size", [256, 4096])
def test_serial_rule_reproduces_reference_blocks(tmp_path, block_size):
    """The data blocks of a build_table.cpu table, rebuilt from the entries
    parsed out of that table."""
    path = table_io.build_table(tmp_path, 3000, block_size, "cpu")
    d = table_io.dump_blocks(path, str(tmp_path / "dump.bin"), verify=True)
    assert d.n > 4 and all(rc == table_io.LDB_OK for rc in d.rc)
    data = d.contents[:-2]                      # then the metaindex and index blocks
    entries = [e for c in data for e in table_io.block_entries(c)]
    assert len(entries) == 3000
    first, blocks = sim.serial_blocks(entries, block_size, 16)
    assert blocks == data
    assert first[-1] == 3000 and len(first) == len(data) + 1
    index = [k for k, _ in table_io.block_entries(d.contents[-1])]
    assert sim.index_keys(entries, first, True) == index


def test_serial_rule_reproduces_the_fixture_tables():
    """Every table lcdb wrote for tests/golden/table_build.bin: blocks and
    index keys (both comparators, every separator and successor edge)."""
    tables = 0
    for s in table_golden_io.read():
        for v in s.variants:
            first, blocks = sim.serial_blocks(s.entries, v.block_size, v.restart_interval)
            assert blocks == v.blocks, s.name
            assert sim.index_keys(s.entries, first, bool(v.internal)) == v.ikeys, s.name
            tables += 1
    assert tables >= 50


def test_parallel_cut_equals_serial_rule():
    rng = random.Random(77)
    for t in range(150):
        n = rng.choice([0, 1, 2, 15, 16, 17, 33, 100, 700]) if t % 3 else rng.randrange(0, 700)
        e = sim.random_entries(rng, n)
        bs = rng.choice([1, 20, 64, 256, 1024, 4096, 65536])
        R = rng.choice([1, 2, 16])
        assert sim.parallel_first(e, bs, R) == sim.serial_blocks(e, bs, R)[0], (t, n, bs, R)


def test_parallel_cut_on_the_fixture_entries():
    for s in table_golden_io.read():
        for v in s.variants:
            want = sim.serial_blocks(s.entries, v.block_size, v.restart_interval)[0]
            assert sim.parallel_first(s.entries, v.block_size, v.restart_interval) == want, s.name
