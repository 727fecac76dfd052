"""Forward scans of decoded blocks on the device:
lgs_block_entries_host and lgs_block_entries_count_dev / _emit_dev against
tools/sim_table_scan.py's serial walk, which tests/test_table_scan_sim.py holds
to what lcdb's own iterator delivered."""
from __future__ import annotations

import os
import struct
import sys

import numpy as np
import pytest

import table_get_golden_io as ggio
import table_golden_io
import table_io

sys.path.insert(0, os.path.join(table_io.ROOT, "tools"))
import sim_block_cut  # noqa: E402
import sim_table_scan as sim  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tab(gpu):
    from lcdb_amd import table
    return table


@pytest.fixture(scope="module")
def sets():
    return table_golden_io.read()


def want(blocks, internal, status=None, walk_from=None, emit_from=None):
    ents, sts = [], []
    for b, blk in enumerate(blocks):
        if status is not None and status[b] != sim.ST_OK:
            ents.append([])
            sts.append(status[b])
            continue
        st, es = sim.block_walk(blk, internal, walk_from[b] if walk_from else None,
                                emit_from[b] if emit_from else None)
        ents.append([(k, v) for _, k, v in es])
        sts.append(st)
    return ents, sts


def on_device(tab, blocks, internal, status=None, walk_from=None, emit_from=None):
    """table.block_entries on uploaded copies: ([entries per block], statuses)."""
    import torch
    dev = torch.device("cuda")
    nb = len(blocks)
    blen = np.array([len(b) for b in blocks], dtype=np.uint32)
    boff = np.zeros(nb, dtype=np.uint64)
    if nb:
        boff[1:] = np.cumsum(blen[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(blocks) + b"\0" * 16, dtype=np.uint8)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)

    def offs(a):
        if a is None:
            return None
        return up(np.array([0xFFFFFFFF if x is None else x for x in a], dtype=np.uint32), np.int32)

    r = tab.block_entries(up(buf, np.uint8), up(boff, np.int64), up(blen, np.int32),
                          int(blen.sum()),
                          None if status is None else up(np.array(status, dtype=np.uint8), np.uint8),
                          offs(walk_from), offs(emit_from), internal)
    torch.cuda.synchronize()
    n = r["n"]
    first = r["entry_first"].cpu().numpy().view(np.uint32)
    assert int(first[nb]) == n and r["keys"].numel() == r["key_bytes"] + 16
    koff, voff = r["key_off"].cpu().numpy(), r["val_off"].cpu().numpy()
    klen, vlen = r["key_len"].cpu().numpy(), r["val_len"].cpu().numpy()
    assert int(koff[n]) == r["key_bytes"] and int(voff[n]) == r["val_bytes"]
    assert r["max_key"] == (int(klen[:n].max()) if n else 0)
    flat = tab._unpack_entries(r["keys"].cpu().numpy(), koff, klen, r["vals"].cpu().numpy(), voff,
                               vlen, n)
    return ([flat[int(first[b]):int(first[b + 1])] for b in range(nb)],
            [int(x) for x in r["status"].cpu().numpy()])


def both(tab, blocks, internal=False, **kw):
    ents, sts = want(blocks, internal, **{k: kw.get(k) for k in ("status", "walk_from", "emit_from")})
    got, gst = tab.block_entries_host(blocks, internal, kw.get("status"), kw.get("walk_from"),
                                      kw.get("emit_from"))
    assert [int(x) for x in gst] == sts
    assert got == ents
    dgot, dst = on_device(tab, blocks, internal, kw.get("status"), kw.get("walk_from"),
                          kw.get("emit_from"))
    assert dst == sts
    assert dgot == ents
    return ents, sts


@pytest.mark.parametrize("internal", [0, 1])
def test_every_fixture_block(tab, sets, internal):
    """Every data block of every fixture table in one call, in the order the
    tables hold them: the entries are the sets' own."""
    blocks, entries = [], []
    for s in sets:
        if int(s.name.endswith("_internal")) != internal:
            continue
        for v in s.variants:
            blocks += v.blocks
            entries += list(s.entries)
    assert len(blocks) > 150
    ents, sts = both(tab, blocks, bool(internal))
    assert all(s == sim.ST_OK for s in sts)
    assert [e for b in ents for e in b] == entries


def block_of(entries, restart_interval=16):
    (blk,) = sim_block_cut.serial_blocks(entries, 1 << 30, restart_interval)[1]
    return blk


def test_long_keys_and_versions(tab):
    """16 KiB keys that share almost everything, and many versions of one user
    key whose shared bytes reach into the tag."""
    big = [(b"p" * 16384 + b"%04d" % i + b"s" * (i % 5), b"v" * (i % 33)) for i in range(20)]
    for r in (16, 3, 1):
        ents, _ = both(tab, [block_of(big, r)])
        assert ents == [big]
    ve = ggio.version_entries()
    for r in (16, 3, 1):
        ents, _ = both(tab, [block_of(ve, r)], True)
        assert ents == [ve]


def test_edge_blocks(tab):
    one = block_of([(b"k", b"v")])
    empty_vals = block_of([(b"a%03d" % i, b"") for i in range(40)], 4)
    sized = block_of([(b"x" * 15, b"1"), (b"x" * 15 + b"y", b"22"), (b"x" * 15 + b"yz", b"333"),
                      (b"y" * 17, b"v" * 15), (b"z" * 16, b"w" * 17)], 2)
    no_restarts = b"\x00\x01\x01kv" + struct.pack("<I", 0)
    too_many = b"\x00\x01\x01kv" + struct.pack("<I", 3)
    blocks = [b"", b"abc", no_restarts, too_many, one, empty_vals, sized, struct.pack("<II", 0, 1)]
    ents, sts = both(tab, blocks)
    assert sts == [0, 0, 1, 0, 1, 1, 1, 1]
    assert ents[4] == [(b"k", b"v")] and len(ents[5]) == 40 and len(ents[6]) == 5
    assert ents[7] == []
    # Internal keys under 8 bytes end the walk where they stand.
    ik = [(b"user%02d" % i + b"\x01" + b"\0" * 7, b"v") for i in range(6)]
    blk = bytearray(block_of(ik, 16))
    eo = table_io.entry_offsets(bytes(blk))
    blk[eo[3]:eo[3] + 2] = b"\x00\x03"
    ents, sts = both(tab, [bytes(blk)], True)
    assert sts == [0] and len(ents[0]) == 3


def test_257_one_entry_blocks_and_none(tab):
    blocks = [block_of([(b"key%05d" % i, b"val%d" % i)]) for i in range(257)]
    ents, sts = both(tab, blocks)
    assert [e[0][0] for e in ents] == [b"key%05d" % i for i in range(257)]
    got, gst = tab.block_entries_host([])
    assert got == [] and len(gst) == 0
    dgot, dst = on_device(tab, [], False)
    assert dgot == [] and dst == []


def test_status_carrying_block(tab):
    blocks = [block_of([(b"a", b"1"), (b"b", b"2")]), block_of([(b"c", b"3")]),
              block_of([(b"d", b"4")])]
    ents, sts = both(tab, blocks, status=[1, 4, 1])
    assert sts == [1, 4, 1] and ents[1] == [] and ents[2] == [(b"d", b"4")]


def hostile_block(n: int) -> bytes:
    """One restart, one 40-byte key, then n - 1 entries with shared = 1: a walk
    back through the entries for each prefix would be quadratic."""
    out = bytes([0, 40, 1]) + b"k" * 40 + b"v"
    for i in range(1, n):
        out += bytes([1, 2, 1]) + struct.pack("<H", i) + b"w"
    return out + struct.pack("<II", 0, 1)


def test_hostile_block_output(tab):
    ents, sts = both(tab, [hostile_block(2000), hostile_block(3)])
    assert sts == [1, 1] and len(ents[0]) == 2000
    assert ents[0][1999] == (b"k" + struct.pack("<H", 1999), b"w")
    # A ramp: every entry extends the one before by a byte, then short ones.
    ramp = bytes([0, 1, 0]) + b"r"
    for i in range(1, 300):
        ramp += bytes([i if i < 128 else (i & 127) | 128]) + (b"" if i < 128 else bytes([i >> 7]))
        ramp += bytes([1, 0]) + bytes([65 + i % 26])
    for i in range(50):
        ramp += bytes([1 + i % 3, 1, 1]) + b"zq"
    ramp += struct.pack("<II", 0, 1)
    ents, sts = both(tab, [ramp])
    assert sts == [1] and len(ents[0]) == 350 and len(ents[0][299][0]) == 300


@pytest.mark.parametrize("internal", [0, 1])
def test_damaged_blocks(tab, sets, internal):
    """The randomly damaged data blocks of test_table_get_sim.damaged_blocks in
    one call, every second one walked and delivered from offsets chosen among
    the headers the model finds; boundary_blocks' headers between
    decode_entry's two paths; with the bytewise ones 20 copies of the hostile
    block with 1 to 5 damaged bytes."""
    import random
    from test_table_get_sim import boundary_blocks, damage_block, damaged_blocks
    rng = random.Random(77 + internal)
    blocks = [d for d, _ in damaged_blocks(sets, bool(internal))]
    assert len(blocks) >= 200
    blocks += [d for d, _ in boundary_blocks(bool(internal))]
    if not internal:
        blocks += [damage_block(rng, hostile_block(2000)) for _ in range(20)]
    walk_from, emit_from = [], []
    for i, d in enumerate(blocks):
        _, heads = sim._headers(d, bool(internal), None)
        wf = ef = None
        if heads and i % 2:
            wf = rng.choice(heads)[0]
            ef = rng.choice([h[0] for h in heads if h[0] >= wf])
        walk_from.append(wf)
        emit_from.append(ef)
    ents, sts = both(tab, blocks, bool(internal), walk_from=walk_from, emit_from=emit_from)
    assert sum(st != sim.ST_OK for st in sts) >= 20 and sum(len(e) for e in ents) > 1000


def test_walk_from_and_emit_from(tab, sets):
    """A block damaged before a later restart point: the walk from restart[0]
    ends at the damage, a walk begun at the later run does not meet it, and
    delivers from the offset asked."""
    s = next(x for x in sets if x.name == "fill4096")
    v = next(v for v in s.variants if (v.block_size, v.restart_interval, v.compression) ==
             (4096, 16, 0))
    blk = bytearray(v.blocks[0])
    eo = table_io.entry_offsets(bytes(blk))
    blk[eo[17]] = 0x64
    blk = bytes(blk)
    full = table_io.block_entries(v.blocks[0])
    ents, sts = both(tab, [blk, blk, blk, v.blocks[0]], walk_from=[None, eo[32], eo[32], eo[16]],
                     emit_from=[None, eo[35], None, eo[20]])
    assert sts == [0, 1, 1, 1]
    assert ents[0] == full[:17] and ents[1] == full[35:] and ents[2] == full[32:]
    assert ents[3] == full[20:]


def test_enospc_reports_sizes_and_writes_nothing(tab):
    blocks = [block_of([(b"key%03d" % i, b"v" * i) for i in range(30)], 4)]
    ents, sts = want(blocks, False)
    n = len(ents[0])
    kb = sum(len(k) for k, _ in ents[0])
    vb = sum(len(v) for _, v in ents[0])
    for caps in ((n - 1, kb, vb), (n, kb - 1, vb), (n, kb, vb - 1), (0, 0, 0)):
        with pytest.raises(tab.ScanError) as e:
            tab.block_entries_host(blocks, caps=caps)
        assert e.value.needed == (n, kb, vb) and e.value.untouched
    got, gst = tab.block_entries_host(blocks, caps=(n, kb, vb))
    assert got == ents and [int(x) for x in gst] == sts
