#!/usr/bin/env python3
"""Generate tests/golden/damage_get.bin and damage_scan.bin from the REFERENCE
table reader on randomly damaged tables.

Run where make_get_golden.py runs: beside the reference checkout, after
oracle/lcdb.mk has compiled it; never on the GPU box.  Uses the two committed
drivers (table_get_driver.c, table_scan_driver.c) as they stand.  A case is a
table of tests/golden/table_build.bin with 1, 1, 2 or 5 seeded one-byte
patches aimed at one class of structure (entry headers, restart arrays, key
bytes, the index block, what ldb_table_open reads, block framing), and what
lcdb's own ldb_table_open, ldb_table_internal_get and table iterator made of
it: a lookup set and three scan runs (the full scan and two seeks).  Nothing
recorded was computed by the code under test.

The damage is seeded by the case's name alone, so a rerun writes the same
bytes.  A case on which the reference driver dies is printed, not recorded,
and replaced by the next seed of its class and table.

Usage: python tests/golden/make_damage_golden.py
"""
from __future__ import annotations

import os
import random
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_get_golden as mg  # noqa: E402
import make_scan_golden as ms  # noqa: E402
import sim_table_get as sim  # noqa: E402
import table_get_golden_io as ggio  # noqa: E402
import table_golden_io  # noqa: E402
import table_scan_golden_io as sgio  # noqa: E402
from damage_golden_io import CLASSES, GET_PATH, SCAN_PATH, SIZE_CAP, TABLES  # noqa: E402
from table_get_golden_io import patched  # noqa: E402
from table_io import entry_offsets  # noqa: E402

PER_PAIR = 2                    # cases per (class, table) where the class has bytes to aim at
LOOKUPS_NEAR, LOOKUPS_WIDE = 20, 16
MAX_DROPPED = 4
RUN_BYTES = 1024               # a run's entries are recorded up to this many bytes
BYTES = (0, 1, 7, 8, 0x7f, 0x80, 0xff)


class Layout:
    """Where the structures of one fixture table lie in its file."""

    def __init__(self, img: bytes, internal: int, bits: int):
        foot = len(img) - 48
        self.footer_varints, at = [], 0
        hs = []
        for _ in range(4):
            v, nxt = sim.varint(img, foot + at, foot + 40, 64)
            self.footer_varints += range(foot + at, nxt)
            hs.append(v)
            at = nxt - foot
        self.magic = list(range(len(img) - 8, len(img)))
        self.meta, self.index = (hs[0], hs[1]), (hs[2], hs[3])
        t = sim.Table(img, False, bool(internal), sim.FILTER_NAME if bits else None)
        assert t.status == sim.ST_OK
        self.data = []                                   # (offset, size) of every data block
        for e in entry_offsets(t.index):
            _, n, vl, p = sim.decode_entry(t.index, e, len(t.index))
            self.data.append(sim.handle_import(t.index[p + n:p + n + vl]))
        self.filter = None
        if bits:
            st, meta = sim.read_block(img, hs[0], hs[1], False)
            _, e = sim.block_seek(meta, sim.FILTER_NAME, False)
            self.filter = sim.handle_import(meta[e[2]:e[2] + e[3]])
        self.img = img

    def raw(self, h) -> bool:
        return self.img[h[0] + h[1]] == 0

    def parts(self, h):
        """Of a block stored raw: (header bytes, first key bytes, key delta
        bytes, value bytes, restart array bytes), as file offsets."""
        off, size = h
        blk = self.img[off:off + size]
        nr = struct.unpack_from("<I", blk, size - 4)[0]
        restarts = size - 4 * (nr + 1)
        head, first, delta, value = [], [], [], []
        for e in entry_offsets(blk):
            _, n, vl, p = sim.decode_entry(blk, e, restarts)
            head += range(off + e, off + p)
            if n:
                first.append(off + p)
            delta += range(off + p, off + p + n)
            value += range(off + p + n, off + p + n + vl)
        return head, first, delta, value, list(range(off + restarts, off + size))


def groups_of(cls: str, lay: Layout):
    """The byte groups class `cls` aims at in this table: [[file offsets]].  A
    patch picks a group, then a byte of it, so a small structure is hit as
    often as a large one."""
    raw = [h for h in lay.data if lay.raw(h)]
    if cls == "entry_headers":
        return [g for h in raw for g in [lay.parts(h)[0] + lay.parts(h)[1]] if g]
    if cls == "restart_arrays":
        return [lay.parts(h)[4] for h in raw]
    if cls == "key_order":
        return [g for h in raw for g in [lay.parts(h)[2]] if g]
    if cls == "index_block":
        if not lay.raw(lay.index):
            return []
        head, _, _, value, restarts = lay.parts(lay.index)
        return [head, value, restarts]
    if cls == "open_time":
        out = [lay.footer_varints, lay.magic, list(range(lay.meta[0], lay.meta[0] + lay.meta[1]))]
        if lay.filter:
            off, size = lay.filter
            last_word = struct.unpack_from("<I", lay.img, off + size - 5)[0]
            out += [list(range(off, off + last_word)), list(range(off + last_word, off + size))]
        return out
    assert cls == "framing"
    out = []
    for h in lay.data + [lay.index]:
        off, size = h
        if not lay.raw(h):
            _, nxt = sim.varint(lay.img, off, off + size, 32)
            out += [list(range(off, nxt)), list(range(off, off + size))]    # the size header, the payload
        out += [[off + size], list(range(off + size + 1, off + size + 5))]   # the type byte, the trailer
    return out


def damage(rng: random.Random, img: bytes, groups, type_bytes):
    """1, 1, 2 or 5 one-byte patches: a type byte becomes 0, 1, 2 or 0xff, any
    other byte one of BYTES or itself with one bit flipped."""
    patches = {}
    for _ in range(rng.choice([1, 1, 2, 5])):
        at = rng.choice(rng.choice(groups))
        if at in type_bytes:
            new = rng.choice([0, 1, 2, 0xff])
        else:
            new = rng.choice(BYTES + (img[at] ^ (1 << rng.randrange(8)),))
        patches[at] = bytes([new])
    return sorted(patches.items())


def block_of_offset(lay: Layout, at: int):
    for b, (off, size) in enumerate(lay.data):
        if off <= at < off + size + 5:
            return b
    return None


def lookups(rng, s, v, lay: Layout, patches):
    """A small lookup set: the queries() neighbourhood of the keys that land in
    a damaged data block, and an even sample of the rest."""
    allq = mg.queries(s.entries, v.ikeys, v.internal, budget=len(s.entries) + 40)
    hit = {block_of_offset(lay, at) for at, _ in patches} - {None}
    near = [k for k in allq if _block_index(v, k) in hit]
    if len(near) > LOOKUPS_NEAR:
        near = near[::-(-len(near) // LOOKUPS_NEAR)]
    wide = allq[::-(-len(allq) // LOOKUPS_WIDE)] + [b""]
    seen, out = set(), []
    for k in near + wide:
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def _block_index(v, key: bytes):
    """The data block the undamaged index sends `key` to, or None."""
    if v.internal and len(key) < 8:
        return None
    for b, ik in enumerate(v.ikeys):
        if sim.compare(key, ik, bool(v.internal)) <= 0:
            return b
    return None


def seeks(s, v, lay: Layout, patches):
    """Two seeks: the first stored key of the first damaged data block (or the
    middle key), and a key a quarter into the table."""
    stored = [k for k, _ in s.entries]
    hit = sorted({block_of_offset(lay, at) for at, _ in patches} - {None})
    a = stored[len(stored) // 2]
    if hit:
        a = next((k for k in stored if _block_index(v, k) == hit[0]), a)
    b = stored[len(stored) // 4]
    if b == a:
        b = stored[-1]
    return [a, b]


def run_get(driver, tmp, table, c, keys):
    try:
        mg.run_driver(driver, tmp, table, c, keys, timeout=60)
    except (AssertionError, struct.error, subprocess.TimeoutExpired) as e:
        return str(e)[:200] or "died"
    return None


def run_scan(driver, tmp, table, c, sk):
    try:
        ms.run_driver(driver, tmp, table, c, sk, timeout=60)
        for r in c.runs:                                  # long runs keep their digest only
            if r.entries and sum(len(k) + len(x) for k, x in r.entries) > RUN_BYTES:
                r.entries = None
    except (AssertionError, struct.error, subprocess.TimeoutExpired) as e:
        return str(e)[:200] or "died"
    return None


def outcome(g, sc):
    return (g.open_rc, [(r.rc, r.called, r.found_key, r.found_value) for r in g.records],
            [(r.rc, r.count, r.digest) for r in sc.runs])


def main() -> None:
    sets = table_golden_io.read()
    gcases, scases, dropped = [], [], []
    per_class = {c: [0, 0] for c in CLASSES}              # recorded, changed
    per_table = {t[0]: [0, 0] for t in TABLES}
    with tempfile.TemporaryDirectory() as tmp:
        gdrv, sdrv = mg.compile_driver(tmp), ms.compile_driver(tmp)
        for tag, sn, want in TABLES:
            s = next(x for x in sets if x.name == sn)
            vi, v = next((i, v) for i, v in enumerate(s.variants) if
                         (v.block_size, v.restart_interval, v.compression, v.bits_per_key) == want)
            lay = Layout(v.file, v.internal, v.bits_per_key)
            type_bytes = {off + size for off, size in lay.data + [lay.index]}
            aims = [(cls, groups_of(cls, lay)) for cls in CLASSES]
            aims = [(cls, g) for cls, g in aims if g]
            # A class with nothing to aim at in this table (entry headers inside
            # compressed blocks) leaves its cases to the classes that have.
            n_cases = {cls: PER_PAIR for cls, _ in aims}
            for i in range(PER_PAIR * (len(CLASSES) - len(aims))):
                n_cases[aims[-1 - i % len(aims)][0]] += 1
            for cls, groups in aims:
                seed = made = 0
                while made < n_cases[cls]:
                    name = f"{cls}:{tag}:{seed}"
                    rng = random.Random(name)
                    seed += 1
                    patches = damage(rng, v.file, groups, type_bytes if cls == "framing" else ())
                    # Damage to the structures is read unverified, so that it
                    # reaches the parsers; framing and open time both ways.
                    both = cls in ("framing", "open_time")
                    verify = (seed & 1) if both else 0
                    paranoid = ((seed >> 1) & 1) if both else 0
                    keys = lookups(rng, s, v, lay, patches)
                    sk = seeks(s, v, lay, patches)
                    mk = lambda C, p: C(name, sn, vi, p, v.internal, v.bits_per_key,  # noqa: E731
                                        paranoid, verify)
                    g, sc = mk(ggio.Case, patches), mk(sgio.Case, patches)
                    table = patched(v.file, patches)
                    died = run_get(gdrv, tmp, table, g, keys) or run_scan(sdrv, tmp, table, sc, sk)
                    if died:
                        print(f"  DROPPED {name}: {died}")
                        dropped.append(name)
                        assert len(dropped) <= MAX_DROPPED
                        continue
                    assert g.open_rc == sc.open_rc
                    g0, s0 = mk(ggio.Case, []), mk(sgio.Case, [])
                    mg.run_driver(gdrv, tmp, v.file, g0, keys)
                    ms.run_driver(sdrv, tmp, v.file, s0, sk)
                    assert g0.open_rc == 0 and s0.runs[0].count == len(s.entries)
                    changed = outcome(g, sc) != outcome(g0, s0)
                    for tally in (per_class[cls], per_table[tag]):
                        tally[0] += 1
                        tally[1] += changed
                    print(f"  {name}: {len(patches)} patches verify={verify} paranoid={paranoid} "
                          f"open={g.open_rc} lookups {sum(r.rc != 0 for r in g.records)}/"
                          f"{len(g.records)} failing, runs " +
                          " ".join(f"{r.rc}/{r.count}" for r in sc.runs) +
                          ("" if changed else "  (outcome unchanged)"))
                    gcases.append(g)
                    scases.append(sc)
                    made += 1
    gsize, ssize = ggio.write(GET_PATH, gcases), sgio.write(SCAN_PATH, scases)
    total = len(gcases)
    changed = sum(c[1] for c in per_class.values())
    print("class            recorded changed")
    for cls, (n, ch) in per_class.items():
        print(f"  {cls:<16}{n:>6}{ch:>8}")
        assert n >= 8, cls
    print("table            recorded changed")
    for tag, (n, ch) in per_table.items():
        print(f"  {tag:<16}{n:>6}{ch:>8}")
        assert n >= 6, tag
    print(f"{total} cases, {changed} change the reference's outcome, {len(dropped)} dropped {dropped}")
    print(f"{GET_PATH}: {sum(len(c.records) for c in gcases)} lookups, {gsize} bytes")
    print(f"{SCAN_PATH}: {sum(len(c.runs) for c in scases)} runs, {ssize} bytes")
    assert 4 * changed >= 3 * total
    assert gsize < SIZE_CAP and ssize < SIZE_CAP


if __name__ == "__main__":
    main()
