"""tools/sim_table_get.py (no GPU): its plain-Python ldb_blockiter_seek and
ldb_table_internal_get reproduce what lcdb's own table reader returned for
every lookup of tests/golden/table_get.bin, and its verdict rule is
version_set.c's save_value."""
from __future__ import annotations

import os
import random
import struct
import sys

import damage_golden_io as dio
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


def test_damage_fixture_covers_the_issue_cases():
    cases, runs = dio.read_get(), dio.read_scan()
    assert os.path.getsize(dio.GET_PATH) < dio.SIZE_CAP
    assert os.path.getsize(dio.SCAN_PATH) < dio.SIZE_CAP
    assert [(c.name, c.patches, c.paranoid, c.verify, c.open_rc) for c in cases] == [
        (c.name, c.patches, c.paranoid, c.verify, c.open_rc) for c in runs]
    sets = table_golden_io.read()
    for c in cases:
        v = next(s for s in sets if s.name == c.set_name).variants[c.variant]
        tag = next(t for t in dio.TABLES if t[0] == dio.table_tag(c))
        assert (c.set_name, (v.block_size, v.restart_interval, v.compression, v.bits_per_key)) == tag[1:]
        assert 1 <= len(c.patches) <= 5 and all(len(new) == 1 for _, new in c.patches)
        assert (c.open_rc == 0) == bool(c.records)
    for cls in dio.CLASSES:
        assert sum(dio.class_of(c) == cls for c in cases) >= 8, cls
    for tag, _, _ in dio.TABLES:
        assert sum(dio.table_tag(c) == tag for c in cases) >= 6, tag
    assert any(c.open_rc for c in cases) and len(cases) >= 90
    for cls in ("open_time", "framing"):
        for flag in ("paranoid", "verify"):
            assert {getattr(c, flag) for c in cases if dio.class_of(c) == cls} == {0, 1}


def test_sim_reproduces_every_damage_record():
    """The model against what lcdb made of the damaged tables: the status of
    ldb_table_open, and per lookup called, status, key and value."""
    sets = table_golden_io.read()
    n = 0
    for c in dio.read_get():
        t = sim.Table(gio.table_of(c, sets), bool(c.paranoid), bool(c.internal),
                      sim.FILTER_NAME if c.bits_per_key else None)
        assert table_io.same_outcome(t.status, c.open_rc), (c.name, t.status, c.open_rc)
        for r in c.records:
            called, st, k, v = t.get(r.key, bool(c.verify))
            assert table_io.same_outcome(st, r.rc), (c.name, r.key[:40], st, r.rc)
            assert called == bool(r.called), (c.name, r.key[:40])
            assert (k, v) == (r.found_key, r.found_value), (c.name, r.key[:40])
            n += 1
    assert n > 1500


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


def damage_block(rng, b: bytes) -> bytes:
    """The damage of the test above: 1, 1, 2 or 5 bytes anywhere in the block."""
    d = bytearray(b)
    for _ in range(rng.choice([1, 1, 2, 5])):
        at = rng.randrange(len(d))
        d[at] = rng.choice([0, 1, 7, 8, 0x7f, 0x80, 0xff, d[at] ^ (1 << rng.randrange(8))])
    return bytes(d)


def damaged_blocks(sets, internal: bool, seed: int = 4242):
    """[(damaged block, [6 to 10 seek targets])] for the GPU block tests: every
    data block of every fill256*, fill4096*, varint* and own_block* table of
    one key kind, damaged once (the large blocks of fill4096* six times and of
    varint* four times, since most of their bytes are values).  The targets
    are keys of the undamaged block, a few of the set's other keys, and their
    k[:-1], k + b"\0" and b"" neighbours.  For internal keys also the version_entries() blocks at
    restart intervals 16, 3 and 1, eight damaged copies each, with
    version_queries."""
    import sim_block_cut
    rng = random.Random(seed + int(internal))
    out = []
    for s in sets:
        if not s.name.startswith(("fill256", "fill4096", "varint", "own_block")):
            continue
        if s.name.endswith("_internal") != internal:
            continue
        copies = 6 if s.name.startswith("fill4096") else (4 if s.name.startswith("varint") else 1)
        some = [k for k, _ in s.entries[::max(1, len(s.entries) // 6)]]
        for v in s.variants:
            for b in v.blocks:
                own = [k for k, _ in table_io.block_entries(b)] + some
                pool = own + [k[:-1] for k in own] + [k + b"\0" for k in own] + [b""]
                pool = sorted(set(pool))
                for _ in range(copies):
                    out.append((damage_block(rng, b),
                                rng.sample(pool, min(len(pool), rng.randint(6, 10)))))
    if internal:
        entries = gio.version_entries()
        for R in (16, 3, 1):
            (blk,) = sim_block_cut.serial_blocks(entries, 1 << 20, R)[1]
            out += [(damage_block(rng, blk), version_queries(entries)) for _ in range(8)]
    return out


def boundary_blocks(internal: bool, seed: int = 128):
    """[(block, [seek targets])]: blocks with an entry whose three header bytes
    OR to exactly 128, the border between decode_entry's one-byte and
    multi-byte paths (block.c:95-104), whole and with damage_block's damage.
    Bytewise: an empty first key with a 128-byte value (header 00 00 80 01).
    Both kinds: a first key of 16 384 bytes (header 00 80 80 01)."""
    import sim_block_cut
    rng = random.Random(seed + int(internal))
    tag = struct.pack("<Q", (5 << 8) | 1) if internal else b""
    user = b"q" * (16384 - len(tag))
    sets = [[(user + tag, b"x"), (user + b"r" + tag, b"yy"), (b"r" * 9 + tag, b"")]]
    if not internal:
        sets.append([(b"", b"v" * 128), (b"a", b"1"), (b"ab", b"v" * 128), (b"b", b"")])
    out = []
    for entries in sets:
        for R in (16, 1):
            (blk,) = sim_block_cut.serial_blocks(entries, 1 << 20, R)[1]
            assert table_io.block_entries(blk) == entries
            assert blk[0] | blk[1] | blk[2] == 128
            keys = [k for k, _ in entries]
            keys += [k[:-1] for k in keys if k] + [k + b"\0" for k in keys]
            out += [(blk, keys)] + [(damage_block(rng, blk), keys) for _ in range(3)]
    return out


def test_boundary_blocks_of_the_gpu_tests():
    import sim_table_scan
    for internal in (False, True):
        batch = boundary_blocks(internal)
        assert batch == boundary_blocks(internal)
        for i, (blk, keys) in enumerate(batch):
            found = sum(_same_seek(blk, k, internal) for k in keys if len(k) >= 8 or not internal)
            assert (sim_table_scan.block_walk_links(blk, internal) ==
                    sim_table_scan.block_walk(blk, internal))
            if i % 4 == 0:                                   # an undamaged one
                assert found >= len(keys) // 2
                assert sim_table_scan.block_walk(blk, internal)[0] == sim.ST_OK


def test_damaged_blocks_of_the_gpu_tests():
    """The batch the GPU block tests use is large enough, and on it the two
    formulations of the seek agree."""
    sets = table_golden_io.read()
    n = 0
    for internal in (False, True):
        blocks = damaged_blocks(sets, internal)
        assert len(blocks) >= 200
        n += len(blocks)
        assert blocks == damaged_blocks(sets, internal)
        for d, keys in blocks:
            assert 6 <= len(keys) <= 10 or (internal and len(keys) == 66)
            for k in keys:
                _same_seek(d, k, internal)
    assert n >= 400


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
