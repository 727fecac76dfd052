"""The CPU models of the block cut and of compaction's output files
(tools/sim_block_cut.py, sim_table_split.py) against what
lcdb's own table builder wrote for the generated sweep
(tests/build_sweep.py, tests/golden/build_sweep.bin), and the sweep against
the edges it is there for.  The edge assertions are computed from the model
and the records, never from the code under test."""
from __future__ import annotations

import hashlib
from collections import Counter

import pytest

import build_sweep as sweep
import build_sweep_golden_io as gio

from sim_block_cut import (index_keys, lcp_of, parallel_first, serial_blocks,  # noqa: E402
                           successor)
import sim_table_split as sim  # noqa: E402

RECORDS = gio.read()
BY_NAME = {r.name: r for r in RECORDS}
NO_SPLIT = sweep.NO_SPLIT


def plain(r) -> bool:
    return (r.compression, r.bits_per_key, r.max_file_size) == (0, 0, NO_SPLIT)


def file_first(r):
    out = [0]
    for n, _, _ in r.files:
        out.append(out[-1] + n)
    return out


def test_records_are_the_case_list():
    cases = sweep.all_cases()
    assert [c.name for c in cases] == [r.name for r in RECORDS]
    for c, r in zip(cases, RECORDS):
        assert (c.spec, c.options()) == (r.spec, r.options()), c.name
    for spec in {r.spec for r in RECORDS if r.spec != "large:1"}:
        assert any(plain(r) for r in RECORDS if r.spec == spec), spec
    assert sum(len(r.files) for r in RECORDS) <= 3000


@pytest.mark.parametrize("r", RECORDS, ids=lambda r: r.name)
def test_model_reproduces_every_record(r):
    es = sweep.entries(r.spec)
    assert (len(es), gio.digest(es)) == (r.count, r.digest)      # the generator is stable
    first, images = sim.split_serial(es, r.block_size, r.restart_interval, r.compression,
                                     r.bits_per_key, bool(r.internal), r.max_file_size)
    assert first == file_first(r)
    assert [(len(i), hashlib.sha256(i).digest()) for i in images] == [f[1:] for f in r.files]
    assert sim.split_blocks(es, r.block_size, r.restart_interval, r.compression,
                            r.max_file_size) == first
    if plain(r):
        assert parallel_first(es, r.block_size, r.restart_interval) == \
            serial_blocks(es, r.block_size, r.restart_interval)[0]


# ---- the sweep reaches the edges ------------------------------------------------

def test_pass_counts():
    """The stride-R prefix ends in either scratch buffer, or makes no pass."""
    for internal in (0, 1):
        got = {sweep.passes(r.count, r.restart_interval) for r in RECORDS if r.internal == internal}
        assert 0 in got and {p & 1 for p in got if p} == {0, 1}, internal
    odd = {r.restart_interval for r in RECORDS} & {3, 5, 7, 17}
    assert odd == {3, 5, 7, 17}
    for r in RECORDS:
        if r.spec.startswith("random"):
            assert r.count == int(r.spec.split(":")[2])
    shapes = {(r.count, r.restart_interval) for r in RECORDS}
    assert {(255, 254), (256, 256), (257, 1000), (2, 3), (1, 1), (513, 17)} <= shapes


def test_exact_blocks_and_their_twins():
    pairs = [p for p in sweep.exact_cases() if p[2] == "block"]
    assert len(pairs) >= 4
    for a, b, _, at in pairs:
        ra, rb = BY_NAME[a.name], BY_NAME[b.name]
        assert rb.block_size == ra.block_size + 1
        es = sweep.entries(a.spec)
        fa, ba = serial_blocks(es, ra.block_size, ra.restart_interval)
        fb, _ = serial_blocks(es, rb.block_size, rb.restart_interval)
        assert 0 < at < len(ba) - 1 and len(ba[at]) == ra.block_size     # flushed at exactly E
        assert fa[:at + 1] == fb[:at + 1] and fb[at + 1] > fa[at + 1]
        assert ra.files != rb.files


def test_exact_files_and_their_twins():
    pairs = [p for p in sweep.exact_cases() if p[2] == "file"]
    assert len(pairs) >= 4 and any(a.compression for a, _, _, _ in pairs)
    for a, b, _, at in pairs:
        ra, rb = BY_NAME[a.name], BY_NAME[b.name]
        assert rb.max_file_size == ra.max_file_size + 1 and at >= 1
        es = sweep.entries(a.spec)
        _, _, start, end = sweep.framed(es, ra.block_size, ra.restart_interval, ra.compression)
        s, e = sweep.file_blocks(start, end, ra.max_file_size)[at]
        assert start[s] > 0 and end[e - 1] - start[s] == ra.max_file_size
        assert ra.files[:at] == rb.files[:at]
        assert ra.files[at][0] < rb.files[at][0]                         # the file gains a block


def test_restart_arrays_with_a_ragged_end():
    """A block of more than R entries whose count is no multiple of R, R odd."""
    hit = set()
    for r in RECORDS:
        R = r.restart_interval
        if plain(r) and R in (3, 5, 7, 17) and not r.spec.startswith("large"):
            first, _ = serial_blocks(sweep.entries(r.spec), r.block_size, R)
            if any(b - a > R and (b - a) % R for a, b in zip(first, first[1:])):
                hit.add(R)
    assert hit == {3, 5, 7, 17}


def test_a_file_holds_raw_and_snappy_blocks():
    """table_builder.c's 12.5 % rule: the trailer's type byte of the model's image."""
    both = 0
    for r in RECORDS:
        if r.compression and r.spec.startswith("mixed") and r.max_file_size == NO_SPLIT:
            es = sweep.entries(r.spec)
            _, (img,) = sim.split_serial(es, *r.options()[:4], bool(r.internal), NO_SPLIT)
            _, _, _, end = sweep.framed(es, r.block_size, r.restart_interval, 1)
            both += {img[e - 5] for e in end} == {0, 1}
    assert both >= 2


def test_filters_over_long_blocks_and_later_files():
    long_block = later_file = 0
    for r in RECORDS:
        if r.bits_per_key and r.spec.startswith("jumbo"):
            _, _, start, end = sweep.framed(sweep.entries(r.spec), r.block_size,
                                            r.restart_interval, r.compression)
            long_block += any(e - s > 4096 for s, e in zip(start, end))
            later_file += any(size > 3 * 2048 for _, size, _ in r.files[1:])
    assert long_block and later_file


def classify(last: bytes, nxt, ikey: bytes) -> str:
    """Why an internal index key is what it is (dbformat.c:232-285)."""
    ua = last[:-8]
    if nxt is None:
        if ikey != last:
            return "successor_shortened"
        return "successor_empty" if not ua else "successor_all_ff" if set(ua) == {0xff} \
            else "successor_kept"
    if ikey != last:
        return "shortened"
    ub = nxt[:-8]
    if ua == ub:
        return "equal_user_keys"
    if ub[:len(ua)] == ua:
        return "prefix"
    d = lcp_of(ua, ub)
    if ua[d] == 0xff:
        return "byte_ff"
    if ua[d] + 1 == ub[d]:
        return "plus_one_is_the_limit"
    assert d + 1 >= len(ua)
    return "not_shorter"


def test_index_key_cases_of_the_binary_sets():
    """Counted over every file of every internal `binary` case: the separators
    between a file's blocks and the successor behind its last block."""
    seen, tagged = Counter(), 0
    for r in RECORDS:
        if not (r.spec.startswith("binary") and r.internal):
            continue
        es = sweep.entries(r.spec)
        ff = file_first(r)
        for a, b in zip(ff, ff[1:]):
            sub = es[a:b]
            first, _ = serial_blocks(sub, r.block_size, r.restart_interval)
            iks = index_keys(sub, first, True)
            assert iks[-1] == successor(sub[-1][0], True)
            for blk, ik in enumerate(iks):
                last = sub[first[blk + 1] - 1][0]
                nxt = sub[first[blk + 1]][0] if blk + 1 < len(iks) else None
                kind = classify(last, nxt, ik)
                seen[kind] += 1
                # The whole-key common prefix runs past the shorter user key:
                # the tag's bytes continue the match (blocks_kernel's min).
                tagged += kind == "prefix" and lcp_of(last, nxt) > len(last) - 8
    for kind in ("shortened", "plus_one_is_the_limit", "prefix", "equal_user_keys",
                 "not_shorter", "successor_all_ff", "successor_empty", "successor_shortened"):
        assert seen[kind] >= 3, (kind, dict(seen))
    # comparator.c:57 also keeps a key whose differing byte is ff.  Between
    # sorted keys that byte is below the limit's, so it is never ff: the
    # branch cannot be reached through the builder, here or in lcdb.
    assert seen["byte_ff"] == 0
    assert tagged >= 3, tagged
