"""The 64 KiB encoder's LDS window (lgs_encode.hip, WinIn) at its edges.

Blocks over 16 896 bytes are encoded by encode_win_kernel<32768>, which keeps
a 32 KiB ring of the chunk in LDS and reads what the ring does not hold --
a probe's 8 bytes, a candidate's 4 bytes, the extension's bytes -- from HBM.
The blocks here put a copy of a chosen length at a chosen distance, so that
those reads fall below the ring, across its lower edge and inside it, and
across the ring's end into its 16-byte mirror; at every alignment of the
chunk's start (sh = address & 15); at the chunk's last dword; in the later
chunks of a block over 64 KiB; with literals of chosen lengths, which this
kernel emits from HBM.  Every block goes through the host batch, the drop-in,
the device batch (1, 2 and 65 blocks a launch) and the device batch at the
case's sh, byte for byte against the reference encoder, and round-trips
through the reference decoder.

The generator (_far): K(12 random) + M + filler + q x 6000 + z + M + tail.
The search that crosses the random filler has a long step when it reaches
the run of q; two of its probes fall into the run, that copy ends at z, and
the next search starts with step 1 on the second M, whose first four bytes
the first search entered at the first M.  The table has 2 048 entries, so
that entry may be overwritten on the way: a case is drawn until the
reference's stream has the copy (test_cases_are_what_they_say proves it for
the bytes each run generates).  To put the first M at a later position, a run
of another byte stands before it: its copy ends one byte before M, so the
search after it enters M's first position.

The ring's lower edge is hu - 32768, hu being a multiple of 4 096 at or after
the matching probe; how far ahead depends on the span of the last batch.
The edge cases do not model hu.  They are a covering sweep: with the second M
at a fixed p and J0 = ceil((p + sh) / 4096) - 8, the first M's first byte is
put at 4096 j + r - sh for j in J0 .. J0 + 2 and r in -5 .. +2, so whichever j
is the edge has the candidate's four bytes below it, across it and above it,
and the other two j have them all out or all in.

A literal before a copy is 1 + (a probe's offset) bytes long (snappy.c:138-
156), and no probe's offset is 4 094, 4 095, 4 096 or 39 999
(test_cases_are_what_they_say asserts it).  The literals of 4 095, 4 096,
4 097 and 40 000 bytes therefore stand after a copy, at the chunk's end
(copy_lit16 through emit_literal).  That copy is a far one where a chunk has
room for both; before a literal of 40 000 bytes it has not.  The literals
before a far copy have the nearest lengths the schedule gives: 4 039 and
4 166 on either side of copy_lit16's 4 096-byte round, 39 507 and 40 742.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np
import pytest

import oracle
from encode_helpers import _device_batch, _elements, _other, _probe_offsets
from lcdb_amd import corpus

RUN = 6000                     # the run that ends the search across the filler
TAIL = 21                      # bytes after the last copy: no probe matches in them
CHUNK = 65536
DISTANCES = (28000, 28672, 32752, 32767, 32768, 32769, 36864, 40000, 49152, 61440, 65000, 65400)
LENGTHS = (4, 63, 64, 65, 200, 5000)


@dataclass
class Case:
    name: str
    data: bytes
    sh: int                    # the chunk start & 15 of the aligned device route
    # what the reference's stream must hold: ("copy", position, length,
    # distance), ("lit", position, length), ("one_literal",),
    # ("no_copy_from", position)
    claims: list = field(default_factory=list)


def _fast(rng: random.Random, n: int, avoid: bytes = b"") -> bytes:
    """n random bytes, none of them zero or in `avoid` (one translate)."""
    bad = set(avoid) | {0}
    good = [b for b in range(256) if b not in bad]
    table = bytes(b if b not in bad else good[b % len(good)] for b in range(256))
    return rng.randbytes(n).translate(table)


def _far(rng: random.Random, dist: int, length: int, pc: int = 12, tail=TAIL,
         pre: int = 0) -> tuple[bytes, int]:
    """A copy of exactly `length` bytes at exactly distance `dist`, its source
    at position pc.  `tail`: a count of random bytes, or the bytes themselves.
    `pre`: random bytes between z and the second M (a probe's offset, so that
    the probe stands on M).  Returns the block and the copy's position."""
    q, q1 = rng.sample(range(1, 256), 2)
    avoid = bytes([q, q1])
    m = _fast(rng, length, avoid)
    head = _fast(rng, 12, avoid)
    if pc != 12:
        assert pc >= 32
        head += bytes([q1]) * (pc - 13) + _other(rng, q, q1, m[0])
    fill = _fast(rng, dist - length - RUN - 1 - pre, avoid)
    z = _other(rng, q, q1, m[0])
    mid = _fast(rng, pre, avoid + m[:1])
    if isinstance(tail, int):
        tail = _fast(rng, tail, avoid)
        if tail:
            tail = _other(rng, q, q1, fill[0]) + tail[1:]
    b = head + m + fill + bytes([q]) * RUN + z + mid + m
    assert len(b) == pc + dist + length
    return b + tail, pc + dist


def _holds(stream: bytes, claims: list, n: int) -> bool:
    """Every claim is true of the stream."""
    el = _elements(stream)
    for c in claims:
        if c[0] == "copy":
            _, pos, length, dist = c
            # the run of copy elements (emit_copy's pieces, snappy.c:75-102)
            # that starts at pos, and no piece at that distance after it
            i = next((i for i, e in enumerate(el) if e[0] == pos and e[2] == dist), None)
            if i is None:
                return False
            got = 0
            while i < len(el) and el[i][2] == dist and el[i][0] == pos + got:
                got += el[i][1]
                i += 1
            if got != length:
                return False
        elif c[0] == "lit":
            if (c[1], c[2], 0) not in el:
                return False
        elif c[0] == "one_literal":
            if el != [(0, n, 0)]:
                return False
        elif c[0] == "no_copy_from":
            if any(e[2] and e[0] + e[1] > c[1] for e in el):
                return False
        else:
            raise AssertionError(c)
    return True


def _build() -> tuple[list[Case], list[tuple[str, int]], dict[str, bytes]]:
    """The cases, the (case, sh) pairs that the aligned route runs besides
    each case's own, and the reference's bytes of every case."""
    rng = random.Random(0x32768)
    ref = oracle.best()
    offs = _probe_offsets(400)
    cases: list[Case] = []
    more: list[tuple[str, int]] = []
    expected: dict[str, bytes] = {}

    def add(name: str, make, sh=None):
        # make() -> (block, claims); drawn until the reference's stream has
        # what the case is about (see the module's docstring).
        for _ in range(4000):
            b, claims = make()
            z = ref.encode(b)
            if _holds(z, claims, len(b)):
                assert len(b) > 16896, name            # the window kernel's class
                expected[name] = z
                # (a case that asks for no sh gets one that is not 0)
                cases.append(Case(name, b, 1 + (7 * len(cases)) % 15 if sh is None else sh, claims))
                return
        raise AssertionError(name)

    def far(dist, length, also=(), **kw):
        def make():
            b, at = _far(rng, dist, length, **kw)
            return b, [("copy", at, length, dist), *also]
        return make

    # ---- 1. far copies by distance and length (and 3. their alignments)
    for length in LENGTHS:
        for dist in DISTANCES + (CHUNK - 12 - length - TAIL,):
            if 12 + dist + length + TAIL > CHUNK:
                continue
            name = f"far_d{dist}_len{length}"
            add(name, far(dist, length))
            if dist in (32768, 61440):
                more += [(name, sh) for sh in range(16) if sh != cases[-1].sh]
    # ---- 2. the ring's lower edge: a covering sweep (the module's docstring)
    p = 36000
    for sh in (0, 5, 15):
        j0 = -(-(p + sh) // 4096) - 8
        for length in (4, 200):
            for dj in range(3):
                for r in range(-5, 3):
                    pc = 4096 * (j0 + dj) + r - sh
                    add(f"edge_sh{sh}_len{length}_j{dj}_r{r}", far(p - pc, length, pc=pc), sh)
    # ---- the ring's end: an unaligned read of ring[W - 7 ..] runs into the
    # 16-byte mirror of ring[0 .. 15].  The probe's 8 bytes (the second M at
    # p + sh = 32768 + r), then the candidate's 4 (the first M there, the
    # second one 7 000 bytes on, where the ring still holds the first).
    for sh in (0, 5, 15):
        for r in range(-7, 1):
            add(f"mirror_probe_sh{sh}_r{r}", far(32768 + r - sh - 12, 64), sh)
        for r in range(-4, 1):
            add(f"mirror_cand_sh{sh}_r{r}", far(7000, 64, pc=32768 + r - sh), sh)
    # ---- 4. the chunk's end and the last dword: n + sh = 0 .. 3 mod 4, and
    # -1, 0, +1, +16 from a multiple of 4 096 (the last staged granule)
    # (a case's name carries nsh = n + sh; its block is n = nsh - sh bytes)
    ends = [38000, 38001, 38002, 38003, 40959, 40960, 40961, 40976]
    gaps = [1, 2, 3, 4, 7, 8, 12, 15, 16, 17, 18, 19, 20, 5, 9, 13]
    for i, (nsh, sh) in enumerate((e, s) for s in (0, 11) for e in ends):
        n = nsh - sh
        length = (20, 63, 64, 65)[i % 4]     # (a copy starts no later than n - 16)
        # a far copy that ends at the chunk's last byte
        add(f"end_copy_nsh{nsh}_sh{sh}", far(n - 70 - 12, 70, tail=0), sh)
        # one that ends t bytes before it, the bytes after it a repeat of
        # position 1: probes past n - 15 must not match
        t = gaps[i]

        def repeat(n=n, t=t, length=length):
            b, at = _far(rng, n - t - length - 12, length, tail=0)
            return b + b[1:1 + t], [("copy", at, length, at - 12)]
        add(f"end_gap{t}_nsh{nsh}_sh{sh}", repeat, sh)
        # a literal of 1 .. 16 bytes after a far copy
        t = 1 + i
        add(f"end_lit{t}_nsh{nsh}_sh{sh}",
            far(n - t - length - 12, length, tail=t, also=[("lit", n - t, t)]), sh)
    for i, t in enumerate(sorted(set(range(1, 21)) - set(gaps))):   # (the gaps not yet taken)
        n = ends[i]

        def repeat(n=n, t=t):
            b, at = _far(rng, n - t - 64 - 12, 64, tail=0)
            return b + b[1:1 + t], [("copy", at, 64, at - 12)]
        add(f"end_gap{t}_nsh{n}_sh0", repeat, 0)
    # ---- 5. blocks over 64 KiB: the ring, the table and the HBM view are
    # the chunk's own
    def in_chunk(k, extra):
        def make():
            c, at = _far(rng, 40000, 200, tail=CHUNK - 12 - 40000 - 200)
            return (rng.randbytes(k * CHUNK) + c + rng.randbytes(extra),
                    [("copy", k * CHUNK + at, 200, 40000)])
        return make
    add("chunk2_far", in_chunk(1, 0))
    add("chunk3_far", in_chunk(2, 100))
    c1 = rng.randbytes(CHUNK)
    add("chunk2_repeats_chunk1", lambda: (c1 + c1[:3000] + rng.randbytes(CHUNK - 3000),
                                          [("no_copy_from", CHUNK)]))
    for t in range(1, 17):
        def tail_chunk(t=t):
            b, at = _far(rng, CHUNK - 64 - 12, 64, tail=0)
            return b + _fast(rng, t), [("copy", at, 64, at - 12), ("lit", CHUNK, t)]
        add(f"tail_chunk{t}", tail_chunk, t - 1)
    # ---- 6. incompressible chunks: every probe of a search that crosses the
    # chunk, the later batches wider than the ring
    for n in (65536, 65535, 32768 + 4096, 16897):
        b = rng.randbytes(n)
        add(f"random{n}", lambda b=b: (b, [("one_literal",)]), 0)
        more.append((f"random{n}", 9))
    fits = [k for k in range(399) if 1 + offs[k] + 8 + 20 + offs[k + 1] - offs[k] <= CHUNK]
    for k in fits[-3:]:
        def first_search(k=k):
            x = _fast(rng, 1 + offs[k])
            return (x + x[1:9] + _fast(rng, 20 + offs[k + 1] - offs[k]),
                    [("copy", 1 + offs[k], 8, offs[k])])
        add(f"first_search_probe{k}", first_search)
    # ---- 7. literals from HBM: copy_lit16's 4 096-byte rounds and its exact
    # tail stores (the lengths: the module's docstring)
    for t in (4095, 4096, 4097, 40000):
        dist = min(40000, CHUNK - 12 - 64 - t)       # (before 40 000 bytes no far copy fits)
        add(f"lit{t}_after_far",
            far(dist, 64, tail=t, also=[("lit", 12 + dist + 64, t)]))
    for k in (175, 176, 249, 250):
        t = 1 + offs[k]
        dist = max(20000, t + RUN + 1000)
        # (a probe is made if the next one is inside the limit)
        add(f"far_after_lit{t}", far(dist, 64, pre=t - 1, tail=TAIL + offs[k + 1] - offs[k],
                                     also=[("lit", 12 + dist - t, t)]))
    # two literals of 16 k + {0, 1, 15} bytes between three far copies, the
    # sources side by side at 12, 16 and 24
    singles = [1 + o for o in offs if (1 + o) % 16 in (0, 1, 15)]
    assert singles[:6] == [1, 15, 16, 17, 31, 32]
    pairs = [(16, 17), (31, 32), (33, 47), (80, 271), (289, 1984)]
    for la, lb in pairs:
        assert la in singles and lb in singles

        def three(la=la, lb=lb):
            q = rng.randrange(1, 256)
            av = bytes([q])
            m1, m2, m3 = _fast(rng, 4, av), _fast(rng, 8, av), _fast(rng, 8, av)
            fill = _fast(rng, 30000, av)
            a = _other(rng, q, m2[0]) + _fast(rng, la - 1, av)
            c = _other(rng, q, m3[0]) + _fast(rng, lb - 1, av)
            head = (_fast(rng, 12, av) + m1 + m2 + m3 + fill + bytes([q]) * RUN
                    + _other(rng, q, m1[0]))
            at1 = len(head)
            at2 = at1 + 4 + la
            at3 = at2 + 8 + lb
            b = (head + m1 + a + m2 + c + m3 + _other(rng, q, fill[0])
                 + _fast(rng, TAIL + lb // 16, av))
            return b, [("copy", at1, 4, at1 - 12), ("lit", at1 + 4, la),
                       ("copy", at2, 8, at2 - 16), ("lit", at2 + 8, lb),
                       ("copy", at3, 8, at3 - 24)]
        add(f"lits{la}_{lb}_between_far", three)
    return cases, more, expected


CASES, MORE, EXPECTED = _build()
BY_NAME = {c.name: c for c in CASES}


def test_cases_are_what_they_say():
    # Each case's claims, read from the reference's stream of the bytes this
    # run generated (not from the generator's word for it).
    ref = oracle.best()
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        z = ref.encode(c.data)
        assert z == EXPECTED[c.name], c.name
        assert c.claims and _holds(z, c.claims, len(c.data)), c.name
        assert ref.decode(z) == c.data, c.name
        assert len(c.data) > 16896, c.name
    # a far copy is one whose source the ring no longer holds: over 28 672
    # bytes back (32 768 less the 4 096 staged ahead)
    for c in CASES:
        if c.name.startswith(("far_d", "end_", "chunk2_far", "chunk3_far", "tail_chunk")):
            assert any(k[0] == "copy" and k[3] >= 28000 for k in c.claims), c.name
    # the sweep's cases: every distance x length that fits, every edge offset
    for length in LENGTHS:
        for dist in DISTANCES:
            assert (f"far_d{dist}_len{length}" in BY_NAME) == (dist + length + 12 + TAIL <= CHUNK)
    for sh in (0, 5, 15):
        for length in (4, 200):
            starts = sorted((BY_NAME[f"edge_sh{sh}_len{length}_j{dj}_r{r}"].claims[0][1]
                             - BY_NAME[f"edge_sh{sh}_len{length}_j{dj}_r{r}"].claims[0][3] + sh)
                            for dj in range(3) for r in range(-5, 3))
            j0 = -(-(36000 + sh) // 4096) - 8
            assert starts == [4096 * (j0 + dj) + r for dj in range(3) for r in range(-5, 3)]
    for sh in (0, 5, 15):
        for r in range(-7, 1):
            assert BY_NAME[f"mirror_probe_sh{sh}_r{r}"].claims[0][1] + sh == 32768 + r
        for r in range(-4, 1):
            _, at, _, dist = BY_NAME[f"mirror_cand_sh{sh}_r{r}"].claims[0]
            assert at - dist + sh == 32768 + r and dist == 7000
    # every sh with the far copies at 32 768 and 61 440
    for name in [c.name for c in CASES if c.name.startswith(("far_d32768_", "far_d61440_"))]:
        assert {BY_NAME[name].sh} | {s for n, s in MORE if n == name} == set(range(16)), name
    assert sum(c.name.startswith("far_d32768_") for c in CASES) == 6
    assert sum(c.name.startswith("far_d61440_") for c in CASES) == 5
    # the chunk's end: (n + sh) & 3 and the last granule
    for sh in (0, 11):
        ns = [len(c.data) + sh for c in CASES if c.name.startswith("end_copy_") and c.sh == sh]
        assert {n & 3 for n in ns} == {0, 1, 2, 3}
        assert {n - 40960 for n in ns} >= {-1, 0, 1, 16}
    assert ({int(c.name[7:].split("_")[0]) for c in CASES if c.name.startswith("end_gap")}
            == set(range(1, 21)))
    assert ({int(c.name[7:].split("_")[0]) for c in CASES if c.name.startswith("end_lit")}
            == set(range(1, 17)))
    # the literal lengths that no search can place before a copy
    lens = {1 + o for o in _probe_offsets(400)}
    assert not lens & {4095, 4096, 4097, 40000}
    assert {4039, 4166, 39507, 40742} <= lens
    # the later batches of the probe table: the last probes that fit a chunk
    ks = sorted(int(c.name[len("first_search_probe"):]) for c in CASES
                if c.name.startswith("first_search_probe"))
    offs = _probe_offsets(400)
    assert len(ks) == 3 and ks == list(range(ks[0], ks[0] + 3)) and ks[0] > 186 + 62
    assert 1 + offs[ks[-1] + 1] + 8 + 20 + offs[ks[-1] + 2] - offs[ks[-1] + 1] > CHUNK
    total = sum(len(c.data) for c in CASES)
    assert total < 20 << 20, total


def _check(outs, names, route):
    ref = oracle.best()
    assert len(outs) == len(names)
    for name, o in zip(names, outs):
        assert o == EXPECTED[name], (route, name)
        assert ref.decode(o) == BY_NAME[name].data, (route, name)


@pytest.mark.gpu
def test_window_host_batch(gpu):
    _check(gpu.encode_batch_host([c.data for c in CASES]), [c.name for c in CASES], "host")


@pytest.mark.gpu
def test_window_dropin(gpu):
    _check([gpu.encode(c.data) for c in CASES], [c.name for c in CASES], "dropin")


def _launches() -> list[tuple[str, list[int]]]:
    """(label, case indices): every case in a launch of 1, 2 or 65 blocks."""
    n = len(CASES)
    out = [("one", [0]), ("two", [1, 2])]
    for at in range(3, n, 65):
        out.append((f"from{at}", [(at + i) % n for i in range(65)]))
    assert {i for _, idx in out for i in idx} == set(range(n))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("label", [lb for lb, _ in _launches()])
def test_window_device_batch(gpu, label):
    idx = dict(_launches())[label]
    _check(_device_batch([CASES[i].data for i in idx]), [CASES[i].name for i in idx], label)


def _device_batch_at(blocks: list[bytes], shs: list[int]) -> list[bytes]:
    """The device batch with block i at an address that is shs[i] mod 16
    (torch's allocations are 256-byte aligned), 16 spare bytes after the last."""
    import torch
    from lcdb_amd import batch
    off = np.zeros(len(blocks), dtype=np.uint64)
    at = 0
    for i, (b, sh) in enumerate(zip(blocks, shs)):
        off[i] = -(-at // 16) * 16 + sh
        at = int(off[i]) + len(b)
    buf = np.zeros(at + 32, dtype=np.uint8)
    for i, b in enumerate(blocks):
        buf[int(off[i]):int(off[i]) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    c = corpus.Corpus(buf, off, np.array([len(b) for b in blocks], np.uint32))
    raw = batch.upload(c)
    assert raw.buf.data_ptr() % 256 == 0
    comp = batch.encode_slots(raw)
    batch.encode(raw, comp)
    torch.cuda.synchronize()
    return batch.to_host(comp).blocks()


@pytest.mark.gpu
@pytest.mark.parametrize("sh", range(16))
def test_window_device_batch_aligned(gpu, sh):
    names = [c.name for c in CASES if c.sh == sh] + [n for n, s in MORE if s == sh]
    assert names
    _check(_device_batch_at([BY_NAME[n].data for n in names], [sh] * len(names)), names, f"sh{sh}")
