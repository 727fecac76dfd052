"""tools/sim_table_get.py (no GPU): its plain-Python ldb_blockiter_seek and
ldb_table_internal_get reproduce what lcdb's own table reader returned for
every lookup of tests/golden/table_get.bin, and its verdict rule is
version_set.c's save_value."""
from __future__ import annotations

import os
import random
import struct
import sys

import table_get_golden_io as gio
import table_golden_io
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_table_get as sim  # noqa: E402


def test_fixture_covers_the_issue_cases():
    cases = gio.read()
    sets = table_golden_io.read()
    plain = {(c.set_name, c.variant) for c in cases if not c.patches}
    assert plain == {(s.name, i) for s in sets for i in range(len(s.variants))}
    names = {c.name.split(":", 1)[1] for c in cases if c.patches}
    for want in ("restart_count_0", "restart_count_over", "block_of_3_bytes",
                 "restart_offset_past_array", "restart_shared_nonzero",
                 "shared_over_previous_key", "varint_into_restart_array", "lengths_over_limit",
                 "internal_key_under_8", "index_value_no_handle", "handle_past_file_end",
                 "unsorted_scan", "unsorted_restart", "flipped_payload_verified",
                 "flipped_payload_unverified"):
        assert want in names, want
    assert os.path.getsize(gio.PATH) < 512 * 1024
    # The corrupting patches do reach the iterator: some lookups fail, some
    # still succeed.
    for c in cases:
        kind = c.name.split(":", 1)[1]
        if c.patches and kind not in ("restart_count_0", "unsorted_scan", "unsorted_restart",
                                      "unsorted_restart_keys", "flipped_payload_unverified"):
            rcs = {r.rc for r in c.records}
            assert 0 in rcs and len(rcs) > 1, c.name


def test_sim_reproduces_every_fixture_record():
    sets = table_golden_io.read()
    n = 0
    for c in gio.read():
        assert c.open_rc == table_io.LDB_OK
        t = sim.Table(gio.table_of(c, sets), bool(c.paranoid), bool(c.internal),
                      sim.FILTER_NAME if c.bits_per_key else None)
        assert t.status == sim.ST_OK, c.name
        for r in c.records:
            called, st, k, v = t.get(r.key, bool(c.verify))
            assert table_io.same_outcome(st, r.rc), (c.name, r.key[:40], st, r.rc)
            assert called == bool(r.called), (c.name, r.key[:40])
            assert (k, v) == (r.found_key, r.found_value), (c.name, r.key[:40])
            n += 1
    assert n > 10000


def _same_seek(block: bytes, key: bytes, internal: bool):
    st, e = sim.block_seek(block, key, internal)
    st2, e2 = sim.block_seek_prefix(block, key, internal)
    assert st == st2, (block[:32], key[:32])
    assert (e is None) == (e2 is None)
    if e is not None:
        assert (e[0], len(e[1]), e[2], e[3]) == e2[:4], (block[:32], key[:32])
    return e is not None


def test_prefix_carrying_seek_equals_the_key_rebuilding_one():
    """The formulation lgs_seek.hip runs against the reference's restated, on
    the fixture's blocks and on randomly damaged copies of them (any block
    contents must give the reference's outcome)."""
    rng = random.Random(99)
    sets = table_golden_io.read()
    hits = n = 0
    for s in sets:
        internal = s.name.endswith("_internal")
        keys = [k for k, _ in s.entries]
        if len(keys) > 40:
            keys = keys[::len(keys) // 40]
        keys += [k[:-1] for k in keys[:8]] + [k + b"\0" for k in keys[:8]] + [b"", b"abc"]
        for v in s.variants[:2]:
            for b in v.blocks[:6]:
                for k in keys:
                    hits += _same_seek(b, k, internal)
                    n += 1
                for _ in range(12):
                    d = bytearray(b)
                    for _ in range(rng.choice([1, 1, 2, 5])):
                        at = rng.randrange(len(d))
                        d[at] = rng.choice([0, 1, 7, 8, 0x7f, 0x80, 0xff, d[at] ^ (1 << rng.randrange(8))])
                    for k in rng.sample(keys, min(6, len(keys))):
                        _same_seek(bytes(d), k, internal)
                        n += 1
    assert hits > 2000 and n > 8000


def version_queries(entries):
    out = []
    for k, _ in entries:
        u, t = k[:-8], struct.unpack("<Q", k[-8:])[0]
        out += [k, u + struct.pack("<Q", t + 1), u + struct.pack("<Q", t - 1),
                u + struct.pack("<Q", t + 256), u + struct.pack("<Q", ((1 << 56) - 1) << 8 | 1),
                u + struct.pack("<Q", 0)]
    return out


def test_shared_bytes_reaching_into_a_tag():
    """Versions of one user key in one block: the tag of the current key lies
    partly in bytes shared with the previous key, which the prefix-carrying
    seek fetches by walking the restart run again."""
    import sim_block_cut
    entries = gio.version_entries()
    for R in (16, 3, 1):
        (blk,) = sim_block_cut.serial_blocks(entries, 1 << 20, R)[1]
        assert table_io.block_entries(blk) == entries
        found = set()
        for k in version_queries(entries):
            if _same_seek(blk, k, True):
                found.add(sim.block_seek(blk, k, True)[1][1])
        assert found == {k for k, _ in entries}


def test_verdict_rule():
    def ik(u, seq, typ):
        return u + struct.pack("<Q", (seq << 8) | typ)
    target = ik(b"user", (1 << 56) - 1, 1)
    assert sim.verdict(ik(b"user", 7, 1), target) == sim.FOUND
    assert sim.verdict(ik(b"user", 7, 0), target) == sim.DELETED
    assert sim.verdict(ik(b"user", 0, 1), target) == sim.FOUND
    assert sim.verdict(ik(b"usez", 7, 1), target) == sim.NOTFOUND
    assert sim.verdict(ik(b"use", 7, 1), target) == sim.NOTFOUND
    assert sim.verdict(ik(b"user\0", 7, 0), target) == sim.NOTFOUND
    assert sim.verdict(ik(b"user", 7, 2), target) == sim.CORRUPT
    assert sim.verdict(ik(b"other", 7, 255), target) == sim.CORRUPT     # the parse comes first
    assert sim.verdict(b"short77", target) == sim.CORRUPT
    assert sim.verdict(ik(b"", 3, 1), ik(b"", 9, 1)) == sim.FOUND
    assert sim.verdict(ik(b"", 3, 0), ik(b"a", 9, 1)) == sim.NOTFOUND
