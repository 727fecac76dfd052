"""The generated sweep of the read side: the tables, the
lookup targets and the scan starts that the recipe
(tests/golden/make_read_sweep_golden.py), the CPU test
(test_read_sweep_sim.py) and the GPU test (test_gpu_read_sweep.py) share.

Nothing is stored here.  A table is a file of a tests/build_sweep.py case, or
of the `versions:<seed>` family below; its entries are regenerated from the
spec and its image by the CPU model (sim_table_split.split_serial), which is
used only after its length and SHA-256 match what lcdb's own builder wrote
(build_sweep.bin, or read_sweep.bin for the versions tables).  The targets of
a table follow from its entries, its block cut and its name alone.
"""
from __future__ import annotations

import functools
import hashlib
import random
import struct
from dataclasses import dataclass

import build_sweep as sweep
import build_sweep_golden_io
from build_sweep import NO_SPLIT, tag
from merge_sweep import S_EDGES

from sim_block_cut import index_keys, serial_blocks  # noqa: E402  (build_sweep put tools/ on the path)
import sim_table_split  # noqa: E402

MAX_SEQ = (1 << 56) - 1
MAX_TAG = tag(MAX_SEQ, 1)
MAX_TARGETS = 700
MAX_SPLIT_CASES = 12
STARTS = 12
FILTERED_SPLITS = ("binary:0:1/b1/r3/c1/f10/m1", "binary:0:0/b1/r5/c0/f30/m1",
                   "random:117:4100:1/b4096/r3/c1/f10/m1")
VERSIONS_SPEC = "versions:1"
# (block_size, restart_interval, compression, bits_per_key)
VERSIONS_OPTIONS = [(1, 16, 0, 0), (256, 1, 0, 0), (256, 2, 0, 0), (256, 3, 0, 0), (4096, 16, 0, 0),
                    (0xffffffff, 64, 0, 0), (256, 3, 0, 10), (4096, 16, 1, 0)]
LONG_CHAIN = 300


@dataclass(frozen=True)
class Table:
    name: str                                       # the case's name, "#file" behind it
    case: str
    spec: str
    file: int
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    internal: int
    max_file_size: int

    @property
    def versions(self) -> bool:
        return self.spec.startswith("versions:")


# ---- the versions family ---------------------------------------------------------

def _versions(seed: int):
    """About 700 internal-key entries whose neighbours share tag bytes: see
    the module docstring of make_read_sweep_golden.py for what each part is for."""
    rng = random.Random(seed)
    tags: dict = {}

    def put(user: bytes, seq: int, typ: int):
        assert 0 <= seq <= MAX_SEQ and typ in (0, 1)
        tags.setdefault(user, set()).add((seq << 8) | typ)

    for seq, typ in ((9, 1), (8, 0), (8, 1), (3, 1)):           # the empty user key
        put(b"", seq, typ)
    for p in range(7):
        # Sequences (j << 8p) | low, j falling: neighbouring tags share the
        # type byte and p sequence bytes.  One type throughout, then equal
        # and unequal types with deletions among them.
        low = rng.randrange(1, 1 << 8 * p) if p else 0
        for j in range(22, 0, -1):
            put(b"eq%d" % p, (j << 8 * p) | low, 1)
        low = rng.randrange(1, 1 << 8 * p) if p else 0
        for j, typ in zip(range(12, 0, -1), (1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 0)):
            put(b"mix%d" % p, (j << 8 * p) | low, typ)
    for c, n in enumerate((2, 3, 5, 17, 40, rng.randrange(2, 41))):    # chains of 2 to 40 versions
        for seq in rng.sample(range(1, 1 << (8, 16, 24, 40, 48, 56)[c]), n):
            put(b"chain%02d" % c, seq, rng.randrange(2))
    for s in S_EDGES + (MAX_SEQ,):
        put(b"edges", s, 1)
        put(b"edges", s - 1, s & 1)
    put(b"edges", MAX_SEQ, 0)
    for n in range(1, 9):
        # A user key that is the previous user key and the leading n bytes of
        # its last (smallest) tag.
        base, seq, typ = b"cont%d" % n, 0x07060504030201 + n, n & 1
        put(base, seq + 0x10000, 1)
        put(base, seq, typ)
        put(base + tag(seq, typ)[:n], seq + 3, 1)
        put(base + tag(seq, typ)[:n], 2, 0)
    for user in (b"seven_7", b"eight__8", b"eight__8x", b"nine____9", b"nine____9\x00"):
        for seq in (0x30201, 0x30101, 7):
            put(user, seq, seq & 1)
    for j in range(LONG_CHAIN, 0, -1):                          # crosses blocks
        put(b"long", j, 0 if j % 10 == 0 else 1)
    keys = [u + struct.pack("<Q", t) for u in sorted(tags) for t in sorted(tags[u], reverse=True)]
    return [(k, (b"val%d." % i)[:i % 11]) for i, k in enumerate(keys)]


@functools.lru_cache(maxsize=2)
def _versions_entries(spec: str):
    return _versions(int(spec.split(":")[1]))


def set_entries(spec: str) -> list:
    """The whole entry set of a spec (build_sweep's, or the versions family)."""
    return _versions_entries(spec) if spec.startswith("versions:") else sweep.entries(spec)


# ---- the tables ------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def sweep_records() -> dict:
    return {r.name: r for r in build_sweep_golden_io.read()}


def _table(c, f: int) -> Table:
    return Table(f"{c.name}#{f}", c.name, c.spec, f, *c.options())


def versions_cases():
    return [sweep.Case(f"{VERSIONS_SPEC}/b{bs}/r{R}/c{comp}/f{bits}/mall", VERSIONS_SPEC, bs, R, comp,
                       bits, 1, NO_SPLIT) for bs, R, comp, bits in VERSIONS_OPTIONS]


@functools.lru_cache(maxsize=1)
def tables() -> list:
    cases = [c for c in sweep.all_cases() if c.spec.split(":")[0] not in ("large", "varint21")]
    out = [_table(c, 0) for c in cases if c.max_file_size == NO_SPLIT]
    splits = [c for c in cases if c.max_file_size != NO_SPLIT]
    chosen = [c for c in splits if c.name in FILTERED_SPLITS]
    assert len(chosen) == len(FILTERED_SPLITS)
    for fam in ("binary", "random", "varint", "mixed", "jumbo"):   # two more of each family
        more = [c for c in splits if c.spec.startswith(fam) and c not in chosen]
        chosen += more[:2] if fam != "random" else more[-1:]
    assert len(chosen) <= MAX_SPLIT_CASES
    recs = sweep_records()
    for c in chosen:
        n = len(recs[c.name].files)
        out += [_table(c, f) for f in sorted({0, n // 2, n - 1})]
    out += [_table(c, 0) for c in versions_cases()]
    cover = lambda f: {f(t) for t in out}                       # noqa: E731
    assert cover(lambda t: t.restart_interval) >= set(sweep.RESTARTS) | {1000}
    assert cover(lambda t: t.block_size) >= set(sweep.BLOCK_SIZES)
    assert cover(lambda t: t.bits_per_key) >= set(sweep.BITS)
    assert cover(lambda t: t.compression) == {0, 1} and cover(lambda t: t.internal) == {0, 1}
    assert len({t.name for t in out}) == len(out)
    return out


def file_range(t: Table):
    """[first, end) of the table's entries in its spec's entry set."""
    if t.versions or t.max_file_size == NO_SPLIT:
        return 0, len(set_entries(t.spec))
    counts = [n for n, _, _ in sweep_records()[t.case].files]
    return sum(counts[:t.file]), sum(counts[:t.file + 1])


def entries(t: Table) -> list:
    a, b = file_range(t)
    es = set_entries(t.spec)
    return es if (a, b) == (0, len(es)) else es[a:b]


def sweep_pin(t: Table):
    """(bytes, SHA-256) of the table as lcdb wrote it (build_sweep.bin)."""
    return sweep_records()[t.case].files[t.file][1:]


@functools.lru_cache(maxsize=2)
def _images(case: str, spec, bs, R, comp, bits, internal, mx):
    return sim_table_split.split_serial(set_entries(spec), bs, R, comp, bits, bool(internal), mx)[1]


def image(t: Table, pin) -> bytes:
    """The model's image of the table, handed out only where its length and
    SHA-256 are lcdb's (`pin`: sweep_pin(t), or the versions table's record)."""
    img = _images(t.case, t.spec, t.block_size, t.restart_interval, t.compression, t.bits_per_key,
                  t.internal, t.max_file_size)[t.file]
    assert (len(img), hashlib.sha256(img).digest()) == tuple(pin), f"{t.name}: not lcdb's file"
    return img


def cut(t: Table):
    """(block_first, raw data blocks, index keys) of the table."""
    es = entries(t)
    first, blocks = serial_blocks(es, t.block_size, t.restart_interval)
    return first, blocks, index_keys(es, first, bool(t.internal))


# ---- the targets -----------------------------------------------------------------

def spaced(items: list, cap: int, seed: str) -> list:
    """All of `items`, or `cap` evenly spaced ones at a seeded phase."""
    n = len(items)
    if n <= cap:
        return list(items)
    r = random.Random(seed).random()
    return [items[int((i + r) * n / cap)] for i in range(cap)]


def bump(k: bytes, at: int, d: int) -> bytes:
    if not k:
        return k
    at %= len(k)
    return k[:at] + bytes([(k[at] + d) & 255]) + k[at + 1:]


# class -> (its share of MAX_TARGETS, targets a stored key gives at most)
QUOTA = {1: {"stored": (200, 1), "neighbours": (80, 4), "word": (78, 14), "seek_tags": (30, 2),
             "tag_step": (40, 2), "tag_byte_step": (70, 14), "type_bytes": (30, 3),
             "user_and_tag": (30, 3), "index": (57, 3)},
         0: {"stored": (300, 1), "neighbours": (130, 4), "word": (118, 14), "index": (75, 3)}}
CLASSES = ("stored", "neighbours", "word", "seek_tags", "tag_step", "tag_byte_step", "type_bytes",
           "user_and_tag", "index", "edges")


def _of_key(cls: str, k: bytes, internal: int) -> list:
    u, t = (k[:-8], k[-8:]) if internal else (k, b"")
    top = MAX_TAG if internal else b""
    if cls == "stored":
        return [k]
    if cls == "neighbours":
        return ([bump(u, -1, 1) + top, bump(u, -1, -1) + top, u[:-1] + top] if u else []) + \
            [u + b"\0" + top]
    if cls == "word":
        return [bump(u, c, d) + top for c in sorted({7, 8, 9, 15, 16, 17, len(u) - 1})
                if 0 <= c < len(u) for d in (1, -1)]
    T = struct.unpack("<Q", t)[0]
    wrap = lambda x: u + struct.pack("<Q", x & ((1 << 64) - 1))     # noqa: E731
    if cls == "seek_tags":
        return [u + MAX_TAG, u + tag(0, 0)]
    if cls == "tag_step":
        return [wrap(T + 1), wrap(T - 1)]
    if cls == "tag_byte_step":
        return [wrap(T + d * (1 << 8 * p)) for p in range(1, 8) for d in (1, -1)]
    if cls == "type_bytes":
        return [u + bytes([x]) + t[1:] for x in (0, 1, 0xff)]
    assert cls == "user_and_tag"
    return [u + t[:n] + MAX_TAG for n in (1, 3, 8)]


@functools.lru_cache(maxsize=256)
def target_classes(t: Table) -> list:
    """[(class, [target])], at most MAX_TARGETS in all.  A target that an
    earlier class has is left out of a later one; the edges stand as they are."""
    es = entries(t)
    stored = [k for k, _ in es]
    first, _, ikeys = cut(t)
    seen, out = set(), []

    def add(cls, keys):
        fresh = []
        for k in keys:
            if k not in seen:
                seen.add(k)
                fresh.append(k)
        out.append((cls, fresh))

    for cls, (share, per) in QUOTA[t.internal].items():
        seed = f"{t.name}/{cls}"
        if cls == "index":
            src = spaced(ikeys, share // per, seed)
            add(cls, [x for k in src for x in (k, bump(k, -1, 1), bump(k, -1, -1))])
        else:
            src = spaced(stored, share // per, seed)
            add(cls, [x for k in src for x in _of_key(cls, k, t.internal)])
    last = stored[-1]
    edges = [b"", (last[:-8] + b"\xff" + MAX_TAG) if t.internal else last + b"\xff"]
    if t.internal:
        edges += [b"abcdefg"[:n] for n in range(8)]                 # under 8 bytes
    edges += [stored[len(stored) // 3]] * 3
    b = (len(first) - 1) // 2                                       # 70 targets in one block
    edges += [stored[first[b] + i % (first[b + 1] - first[b])] for i in range(70)]
    out.append(("edges", edges))
    assert sum(len(ks) for _, ks in out) <= MAX_TARGETS, t.name
    return out


def targets(t: Table) -> list:
    return [k for _, ks in target_classes(t) for k in ks]


def starts(t: Table) -> list:
    """The scan starts: the first target of each class, then stored keys at
    the quarter points (and the eighths, where classes are few)."""
    stored = [k for k, _ in entries(t)]
    out = [ks[0] for _, ks in target_classes(t) if ks]
    out += [stored[len(stored) * q // 8] for q in (2, 4, 6, 1, 3, 5, 7)]
    uniq = []
    for k in out:
        if k not in uniq:
            uniq.append(k)
    return uniq[:STARTS]


# ---- what a recorded outcome means ---------------------------------------------

def tag_bytes_shared(t: Table, first: list, es: list, ordinal: int) -> int:
    """How many bytes of its own tag the stored entry's `shared` count covers:
    the bytes lgs_seek.hip's key_bytes fetches from earlier entries (0 at a
    restart point and for bytewise keys)."""
    import bisect
    if not t.internal:
        return 0
    b = bisect.bisect_right(first, ordinal) - 1
    if (ordinal - first[b]) % t.restart_interval == 0:
        return 0
    prev, key = es[ordinal - 1][0], es[ordinal][0]
    n = 0
    while n < min(len(prev), len(key)) and prev[n] == key[n]:
        n += 1
    return max(0, n - (len(key) - 8))


def conditions(tables, records) -> dict:
    """The class counts of a fixture: what the recipe and the CPU test assert."""
    import collections
    import sim_table_get
    from read_sweep_golden_io import CALLED, REFUSED
    n = collections.Counter()
    for t, r in zip(tables, records):
        es = entries(t)
        first = cut(t)[0]
        keys = [k for k, _ in es]
        for k, rc, fl, o in zip(targets(t), r.rc, r.flags, r.ordinal):
            if t.internal and len(k) < 8:
                n["short"] += 1
                continue
            if fl & REFUSED:
                n["refused"] += 1
            elif not fl & CALLED and rc == 0 and \
                    sim_table_get.compare(keys[-1], k, bool(t.internal)) >= 0:
                n["between"] += 1
            if fl & CALLED:
                n["shared", tag_bytes_shared(t, first, es, o)] += 1
    return n


def check_conditions(n) -> None:
    assert n["refused"] >= 1000, n
    assert n["between"] >= 1000, n
    assert n["shared", 1] >= 200, n
    for p in range(1, 7):
        assert n["shared", p + 1] >= 20, (p, n)
    assert n["short"] >= 30, n
