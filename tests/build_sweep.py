"""The generated sweep of the device table builder: the
case list and the seeded entry-set generator that the recipe
(tests/golden/make_build_sweep_golden.py), the CPU test
(test_build_sweep_sim.py) and the GPU test (test_gpu_build_sweep.py) share.

An entry set is named by a spec string and regenerated from it, never stored:
    binary:<prefix length>:<internal>     user keys over 00 61 62 fe ff
    random:<seed>:<n>:<internal>          sim_block_cut.random_entries
    varint:<internal>                     lengths on both sides of 2^7 and 2^14
    varint21                              values of 2^21 - 1 and 2^21 bytes
    mixed:<seed>:<n>:<internal>           stretches of random and of repeated values
    jumbo:<internal>                      tiny entries around a few 5-70 KB values
    large:<internal>                      2^20 + 4099 counters
A case is a spec with the builder's options.  The exact cases (a block whose
estimate equals block_size, a file whose data bytes equal max_file_size, and
their + 1 twins) are resolved from the CPU model (tools/sim_block_cut.py,
sim_table_split.py), which the fixture pins to lcdb.
"""
from __future__ import annotations

import functools
import os
import random
import struct
import sys
from dataclasses import dataclass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

NO_SPLIT = (1 << 64) - 1
RESTARTS = [1, 2, 3, 5, 7, 16, 17, 64]
BLOCK_SIZES = [1, 64, 256, 4096, 0xffffffff]
BITS = [0, 1, 10, 30]
ALPHABET = b"\x00\x61\x62\xfe\xff"
PREFIX = b"\xfeP\x00refix\xff-of-17-b"           # cut at 0, 7, 8, 9 or 17 bytes
LARGE_N = (1 << 20) + 4099


@dataclass(frozen=True)
class Case:
    name: str
    spec: str
    block_size: int
    restart_interval: int
    compression: int
    bits_per_key: int
    internal: int
    max_file_size: int

    def options(self):
        return (self.block_size, self.restart_interval, self.compression, self.bits_per_key,
                self.internal, self.max_file_size)


def tag(seq: int, typ: int) -> bytes:               # dbformat.h: pack_seqtype, fixed64
    return struct.pack("<Q", (seq << 8) | typ)


def passes(n: int, R: int) -> int:
    """Doublings of R below n: the stride-R prefix's pass count."""
    p, step = 0, R
    while step < n:
        p, step = p + 1, step * 2
    return p


# ---- the entry-set families --------------------------------------------------

def _suffixes():
    out = [b""]
    for ln in (1, 2, 3):
        out += [bytes(ALPHABET[(i // 5 ** d) % 5] for d in range(ln)) for i in range(5 ** ln)]
    rng = random.Random(4)
    out += [bytes(ALPHABET[(i // 5 ** d) % 5] for d in range(4))
            for i in sorted(rng.sample(range(625), 144))]
    return out                                      # every suffix of 0-3 bytes, 144 of 4: 300


def _binary(plen: int, internal: int):
    users = sorted(PREFIX[:plen] + s for s in _suffixes())
    if not internal:
        return [(u, b"v%d" % i * (i % 7)) for i, u in enumerate(users)]
    out = []
    for i, u in enumerate(users):
        nv = 1 + (i % 3 == 0) + (i % 7 == 0)
        nxt = users[i + 1] if i + 1 < len(users) else b""
        # Where the next user key is this one and a 00 byte and more, the last
        # version is a deletion (tag byte 00) whose sequence continues the
        # match: the whole-key common prefix is longer than this user key.
        follow = len(nxt) > len(u) and nxt[:len(u)] == u and nxt[len(u)] == 0 and i % 2 == 0
        for v in range(nv):
            low, typ = 0x33, (i + v) & 1
            if follow and v == nv - 1:
                typ = 0
                low = nxt[len(u) + 1] if len(nxt) > len(u) + 1 else 1
            out.append((u + tag((i + 1) * 0x10000 + (nv - 1 - v) * 0x100 + low, typ),
                        b"val%d." % i * ((i + v) % 5)))
    return out


def _random(seed: int, n: int, internal: int):
    from sim_block_cut import random_entries
    rng = random.Random(seed)
    es = random_entries(rng, n)
    if not internal:
        return es
    out = []
    for i, (u, v) in enumerate(es):                 # 1-3 versions, sequence falling
        for j in range(rng.choice([1, 1, 2, 3])):
            out.append((u + tag(5 * (n - i) + 3 - j, rng.randrange(2)), v[:len(v) >> j]))
    return out[:n]


def _varint(internal: int):
    edges = [127, 128, 16383, 16384]
    vals = [0, 127, 128, 16383, 16384, 1]
    out = []
    for g, L in enumerate(edges):
        p = bytes([0x30 + g]) * L                   # shared: L; non-shared: 1, L - 1, L, L + 1
        for k in (p + b"a", p + b"b", p + b"c" + b"x" * (L - 2), p + b"d" + b"y" * (L - 1),
                  p + b"e" + b"z" * L):
            i = len(out)
            v = bytes((i * 7 + t) & 255 for t in range(256)) * 65
            out.append((k + (tag(900 - i, i & 1) if internal else b""), v[:vals[i % len(vals)]]))
    return out


def _varint21():
    body = bytes(range(256)) * 8193
    return [(b"k0", body[:(1 << 21) - 1]), (b"k1", body[1:(1 << 21) + 1]), (b"k2", b"tail")]


def _mixed(seed: int, n: int, internal: int):
    rng = random.Random(seed)
    out, noisy, left = [], True, 0
    for i in range(n):
        if left == 0:
            noisy, left = not noisy, rng.randrange(1, 40)
        left -= 1
        ln = rng.randrange(0, 301)
        v = rng.randbytes(ln) if noisy else (b"word%d " % (i % 3) * 60)[:ln]
        k = b"mixed/%05d/%s" % (2 * i, b"abc"[:i % 4])
        out.append((k + (tag(7000 + i, 1 if i % 9 else 0) if internal else b""), v))
    return out


def _jumbo(internal: int):
    big = {40: 5000, 41: 70000, 700: 33000, 1499: 20000}
    rng = random.Random(11)
    out = []
    for i in range(1500):
        v = rng.randbytes(big[i]) if i in big else b"xyz"[:i % 4]
        out.append((b"j%04d" % i + (tag(i + 1, 1) if internal else b""), v))
    return out


def _large(internal: int):
    pack, packv = struct.Struct(">Q").pack, struct.Struct("<I").pack
    if internal:
        return [(pack(i) + tag(i + 1, 1), packv(i * 2654435761 & 0xffffffff)[:i % 5])
                for i in range(LARGE_N)]
    return [(pack(i), packv(i * 2654435761 & 0xffffffff)[:i % 5]) for i in range(LARGE_N)]


_FAMILIES = {"binary": _binary, "random": _random, "varint": _varint, "varint21": _varint21,
             "mixed": _mixed, "jumbo": _jumbo, "large": _large}


@functools.lru_cache(maxsize=8)
def _entries(spec: str):
    name, *args = spec.split(":")
    return _FAMILIES[name](*(int(a) for a in args))


def entries(spec: str) -> list:
    """The entry set of a spec: sorted (key, value) pairs.  Shared, not to be changed."""
    return _entries(spec)


# ---- the cases ------------------------------------------------------------------

def _static_cases():
    out = []

    def case(spec, bs, R, comp, bits, mx):
        internal = int(spec.split(":")[-1]) if ":" in spec else 0
        mxs = "all" if mx == NO_SPLIT else str(mx)
        out.append(Case(f"{spec}/b{bs}/r{R}/c{comp}/f{bits}/m{mxs}", spec, bs, R, comp, bits,
                        internal, mx))

    def plain(spec, bs, R):
        """No compression, no filter, one file: the image fixes the raw blocks
        and the index keys."""
        case(spec, bs, R, 0, 0, NO_SPLIT)

    # binary: every prefix length, bytewise and internal.
    for j, plen in enumerate((0, 7, 8, 9, 17)):
        for internal in (0, 1):
            spec = f"binary:{plen}:{internal}"
            plain(spec, 1, RESTARTS[(2 * j + internal) % 8])
            plain(spec, 256, RESTARTS[(2 * j + internal + 3) % 8])
            case(spec, 64, RESTARTS[(j + 2) % 8], 1, BITS[(j + internal) % 4], 2000 + 700 * j)
    case("binary:0:1", 1, 3, 1, 10, 1)              # every entry a file: the successors
    case("binary:0:0", 1, 5, 0, 30, 1)
    case("binary:17:1", 100, 7, 1, 1, 1)

    # random: n across workgroup and scan-tile edges, R odd, n - 1, n and above n.
    shapes = [(1, 1), (2, 1), (2, 2), (2, 3), (5, 5), (8, 7), (17, 17), (18, 17), (65, 64),
              (255, 254), (256, 256), (257, 1000), (255, 3), (256, 5), (257, 7), (513, 17),
              (513, 2), (4100, 3), (4099, 5), (4100, 64), (4101, 16), (4100, 7)]
    for j, (n, R) in enumerate(shapes):
        internal = j & 1 if n > 1 else 0
        spec = f"random:{100 + j}:{n}:{internal}"
        bs = BLOCK_SIZES[j % 5]
        plain(spec, bs, R)
        bs2 = BLOCK_SIZES[(j + 2) % 5]
        small = n <= 260 or bs2 >= 4096
        mx = [1 if small else 40000, 3000 if n <= 600 else 60000, NO_SPLIT][j % 3]
        case(spec, bs2, R, (j + 1) & 1, BITS[j % 4], mx)
    case("random:117:4100:1", 4096, 3, 1, 10, 1)    # filters in every file of a long split
    case("random:113:256:1", 0xffffffff, 5, 1, 30, 1)

    # varint: the length edges at R = 1, 3 and 17 and in small blocks.
    for internal in (0, 1):
        spec = f"varint:{internal}"
        for R, bs in ((1, 1), (3, 200), (17, 20000)):
            plain(spec, bs, R)
            case(spec, bs, R, 1, BITS[(R + internal) % 4], [1, 40000, NO_SPLIT][R % 3])
    plain("varint21", 4096, 3)
    case("varint21", 0xffffffff, 1, 1, 10, NO_SPLIT)

    # mixed: raw and snappy blocks in one file.
    for j, (n, internal) in enumerate(((400, 0), (400, 1), (513, 1))):
        spec = f"mixed:{30 + j}:{n}:{internal}"
        plain(spec, 256, RESTARTS[j + 2])
        case(spec, 1024, RESTARTS[j + 3], 1, BITS[j + 1], NO_SPLIT)
        case(spec, 4096, RESTARTS[j + 4], 1, 10, 20000)

    # jumbo: blocks of one entry and of hundreds, filters over blocks far past 2 KiB.
    for internal in (0, 1):
        spec = f"jumbo:{internal}"
        plain(spec, 4096, 5 if internal else 17)
        case(spec, 4096, 7, 1, 10, 30000)
        case(spec, 256, 3, 0, 30 if internal else 1, 1 if internal else NO_SPLIT)

    # large: the kernels' own loops past their grid caps.
    plain("large:0", 4096, 7)
    case("large:1", 4096, 7, 1, LARGE_FILTER_BITS, 1 << 20)
    return out


# The filtered large case: the model's filter blocks for 2^20 keys take about
# 4 s of CPU, so the filter stays on.
LARGE_FILTER_BITS = 10

# (spec, R, compression, the size the search starts from)
EXACT_BLOCKS = [("binary:8:1", 3, 0, 200), ("random:112:255:0", 5, 1, 700),
                ("mixed:31:400:1", 7, 0, 1000), ("random:114:257:0", 17, 0, 500),
                ("jumbo:0", 17, 1, 3000), ("binary:17:0", 64, 0, 300)]
# (spec, block_size, R, compression, bits_per_key, the size the search starts from)
EXACT_FILES = [("binary:9:1", 64, 5, 0, 10, 1500), ("random:112:255:0", 256, 3, 1, 0, 3000),
               ("mixed:31:400:1", 512, 17, 1, 10, 4000), ("jumbo:1", 300, 7, 1, 0, 2500),
               ("random:119:4100:1", 1024, 2, 0, 1, 50000)]


def framed(es, block_size, R, compression):
    """(block_first, blocks, start, end): one cut framed from offset 0."""
    import oracle
    from sim_block_cut import serial_blocks
    first, blocks = serial_blocks(es, block_size, R)
    _, hoff, hsize, _ = oracle.table_write_blocks(blocks, compression, 0)
    return first, blocks, [int(x) for x in hoff], [int(o) + int(s) + 5 for o, s in zip(hoff, hsize)]


def file_blocks(start, end, max_size):
    """[(first block, block after the last)] of the files (db_impl.c:1417-1425)."""
    out, s = [], 0
    while s < len(start):
        b = s
        while b + 1 < len(start) and end[b] - start[s] < max_size:
            b += 1
        out.append((s, b + 1))
        s = b + 1
    return out


def exact_block(spec, R, base):
    """(E, b): the first size E >= base under which a block b that is neither
    first nor last is flushed with its estimate exactly E, and the lowest such b."""
    from sim_block_cut import serial_blocks
    es = entries(spec)
    for E in range(base, base + 4096):
        _, blocks = serial_blocks(es, E, R)
        for b in range(1, len(blocks) - 1):
            if len(blocks[b]) == E:                 # the finished size is the estimate at the flush
                return E, b
    raise AssertionError(f"{spec}: no exact block from {base}")


def exact_file(spec, bs, R, comp, base):
    """(M, f): the first max_file_size M >= base under which a file f that is
    neither first nor last holds exactly M data bytes, and the lowest such f."""
    _, _, start, end = framed(entries(spec), bs, R, comp)
    for M in range(base, base + 8192):
        fb = file_blocks(start, end, M)
        for f in range(1, len(fb) - 1):
            s, e = fb[f]
            if end[e - 1] - start[s] == M:
                return M, f
    raise AssertionError(f"{spec}: no exact file from {base}")


@functools.lru_cache(maxsize=1)
def exact_cases():
    """[(exact Case, its + 1 twin, "block" or "file", index of the block or file)]."""
    out = []
    for spec, R, comp, base in EXACT_BLOCKS:
        E, b = exact_block(spec, R, base)
        internal = int(spec.split(":")[-1])
        mk = lambda bs, nm: Case(f"{spec}/r{R}/c{comp}/{nm}", spec, bs, R, comp, 0, internal,  # noqa: E731
                                 NO_SPLIT)
        out.append((mk(E, "block_exact"), mk(E + 1, "block_exact_plus_1"), "block", b))
    for spec, bs, R, comp, bits, base in EXACT_FILES:
        M, f = exact_file(spec, bs, R, comp, base)
        internal = int(spec.split(":")[-1])
        mk = lambda mx, nm: Case(f"{spec}/b{bs}/r{R}/c{comp}/{nm}", spec, bs, R, comp, bits,  # noqa: E731
                                 internal, mx)
        out.append((mk(M, "file_exact"), mk(M + 1, "file_exact_plus_1"), "file", f))
    return out


@functools.lru_cache(maxsize=1)
def all_cases():
    out = _static_cases()
    for a, b, _, _ in exact_cases():
        out += [a, b]
    assert len({c.name for c in out}) == len(out)
    return out
