"""The wave and wide decoders' LDS images (lgs_decode.hip) at their edges.

decode_kernel<4608> / <16896> decode in place: the stream is staged at the
top of the LDS buffer that the output grows into, and every op writes 64
lanes.  An op is in place while S = made_before + slen - lm stays under a
bound that depends on the class and on the alignment of stream and output;
a stream over it is decoded again from global memory.  Family A puts S at
every integer around that bound (a covering sweep: the test does not know
the alignment terms), with each kind of op as the one that attains it, at
sixteen alignments, at the staging limit, and through the drop-in.

decode_wide_kernel<32768, 4096> keeps a 32 KiB output ring flushed in
16-byte granules and a 4 KiB stream ring with a mirror, refilled 2 KiB at a
time; copies further back than the ring read flushed output from HBM; long
literals bypass the stream ring, which is then staged again.  Family B puts
copies at and around the far distance, runs of far copies across flushes,
block ends at each output alignment, tags of every form across each refill
edge, long literals of the edge lengths, their end offsets swept across the
refill edges, overlapping copies across the output ring's wrap, and every
reject after the ring has wrapped.

Family C sends the far-copy, long-literal and reject pools, and a block of
0xffffff bytes, to decode_pair_kernel above its usual 4 608 bytes.

Every expected status and byte is the reference's (oracle.best()).  The
kernel's constants are used to place cases, never asserted.
test_cases_are_what_they_say (no device) recomputes from each stream's bytes
what the case claims and holds the covering ranges complete.

Where the issue's lists would not fit 40 MB of streams as a full cross
(fillers are random literals, so a case at output position 32 768 costs that
many stream bytes), the cross is thinned by rotation, and the docstrings of
the builders say how: B1's wrap placements alternate the copy form, B8 takes
three of the nine distances at each position.
"""
from __future__ import annotations

import os
import random
import time
from dataclasses import dataclass, field

import numpy as np
import pytest

import oracle
from decode_helpers import Stream, _header, _lit_header, _varint, run_ahead, walk

PROBE = os.environ.get("LGS_TEST_PROBE") == "1"

CLASSES = {4608: 5168, 16896: 17648}       # the class -> B of the in-place bound (placing only)
STAGE = {4608: 5232, 16896: 17712}         # the class -> the longest staged stream (placing only)
A1_RANGE, A2_RANGE, A3_RANGE = (-64, 48), (-40, 24), (-32, 24)
A2_KINDS = ("copy2", "copy4", "overlap", "lit60", "lit61_64", "litlong", "copy2_lit", "copy4_lit")
FAR_DISTS = (32640, 32703, 32704, 32705, 32706, 32767, 32768, 32769)
FAR_LENS = (1, 4, 63, 64)
EDGES = (2048, 4096, 6144, 8192)
B4_WANTS = (16897, 24575, 24577, 32767, 32768, 32769, 65535, 65536, 65537, 66048, 66049,
            98303, 98305)
B6_LENS = (65, 79, 80, 81, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 32767,
           32768, 32769, 40000, 65536)
B6_RESIDUE_LENS = (65, 4097, 12289)
B7_M = (4096, 6144, 8192)
B8_DISTS = (1, 2, 3, 5, 8, 15, 16, 17, 63)
OSH3, ISH3 = (0, 5, 15), (0, 7, 15)
DROPIN_MIN, DROPIN_MAX = 16897, 66048


@dataclass
class Case:
    name: str
    fam: str
    s: bytes
    cap: int
    out: bytes | None          # the builder's own output; None: a reject
    osh: int = 0               # output address & 15 on the device route
    ish: int = 0               # input address & 15 on the device route
    claim: dict = field(default_factory=dict)


# ---------------------------------------------------------------------------
# Family A
# ---------------------------------------------------------------------------
def _r_wanted(cls: int, S: int) -> int:
    """The bound on S moves with the stream's length: r = (STAGE - slen) & 15
    is taken off it, and a builder that tunes S by the length of the tail
    moves S and the bound together.  So the last 64-byte copy is shortened
    by delta bytes and the tail lengthened by as many: S stays, slen and r
    change.  With r = -2 (S - B) mod 16 the excess S - (B - r) takes every
    integer from min(S) - B + 15 to max(S) - B as S runs through a range
    (test_cases_are_what_they_say holds that too)."""
    return (-2 * (S - CLASSES[cls])) & 15


def _a1(rng, cls: int, S: int, v: int) -> Case:
    """The run-ahead family: a 4-byte literal, N 64-byte COPY2s at dist 4,
    then k 1-byte literals; a 1-byte literal with a 2-byte header and a
    4-byte COPY1 (stream cost 3 and 2 for 1 and 4 bytes) give S its other
    parity and a third element.  S is attained at the first 1-byte literal:
    S = 3 + 64 N + T, T the stream bytes from that literal on."""
    T0 = 1300 if cls == 4608 else 1800
    N = (S - 3 - T0) // 64
    c = 1 if (v % 2 == 1) else 0                # a COPY1 in every second stream
    for delta in range(16):                     # (see _r_wanted)
        T = S - 3 - 64 * N + delta
        e = T & 1                               # one 3-byte element for an odd T
        k = (T - 3 * e - 2 * c) // 2
        want = 4 + 64 * N - delta + k + 4 * c + e
        if (STAGE[cls] - (len(_varint(want)) + 5 + 3 * N + T)) & 15 != _r_wanted(cls, S):
            continue
        s = Stream(rng).lit(4)
        for _ in range(N - 1):
            s.copy(64, 4)
        s.copy(64 - delta, 4)
        for _ in range(k):
            s.lit(1)
        if c:
            s.copy(4, 1, form=1)
        if e:
            s.lit(1, hdr=2)
        out = s.done()
        if (STAGE[cls] - len(out)) & 15 == _r_wanted(cls, S):
            return Case(f"A1_c{cls}_S{S}", "A1", out, cls, bytes(s.out), claim=dict(S=S, cls=cls))
    raise AssertionError((cls, S))


def _a2(rng, cls: int, S: int, kind: str) -> Case:
    """Op X of the given kind attains S: 64-byte copies bring made up, X
    follows, then a 1-byte literal with a 3-byte header (so the op after X is
    below it) and 1-byte literals, of which made - lm falls by one each.

    copy2_lit / copy4_lit: the 1-byte copy X is followed at once by a plain
    1-byte literal, which attains the same S.  The copy's 63 wild lanes are
    written after the next tag has been parsed (the deferred write), so the
    first stream byte that a copy over the bound can spoil is that literal's
    data byte, two bytes past the copy's tag."""
    tight = kind.endswith("_lit")
    x_n = dict(copy2=1, copy4=1, copy2_lit=1, copy4_lit=1, overlap=2, lit60=37, lit61_64=61 + S % 4, litlong=100 + S % 90)[kind]
    x_data = x_n if kind.startswith("lit") else 0
    for delta in range(48):
        c = _a2_delta(rng, cls, S, kind, delta, tight, x_n, x_data, dry=True)
        if (STAGE[cls] - c) & 15 == _r_wanted(cls, S):
            c = _a2_delta(rng, cls, S, kind, delta, tight, x_n, x_data)
            assert (STAGE[cls] - len(c.s)) & 15 == _r_wanted(cls, S)
            return c
    raise AssertionError((cls, S, kind))


def _a2_delta(rng, cls, S, kind, delta, tight, x_n, x_data, dry=False):
    N = (cls - 64) // 64
    while True:
        made_b = 4 + 64 * N - delta
        rest = S - made_b - x_data - (0 if tight else 4)   # stream bytes of the 1-byte literals
        e = rest & 1
        k = (rest - 3 * e) // 2
        if k >= 1 and made_b + x_n + 1 + k + e <= cls:
            break
        N -= 1
        assert N > 0
    if dry:                                     # the stream's length, without building it
        want = made_b + x_n + (0 if tight else 1) + k + e
        x_tag = dict(copy2=3, copy4=5, copy2_lit=3, copy4_lit=5, overlap=3, lit60=1, lit61_64=2,
                     litlong=2)[kind]
        return len(_varint(want)) + 5 + 3 * N + x_tag + x_data + (0 if tight else 4) + 2 * k + 3 * e
    s = Stream(rng).lit(4)
    for _ in range(N - 1):
        s.copy(64, 4)
    s.copy(64 - delta, 4)
    if kind in ("copy2", "copy2_lit"):
        s.copy(1, 777)
    elif kind in ("copy4", "copy4_lit"):
        s.copy(1, 777, form=3)
    elif kind == "overlap":
        s.copy(2, 1)
    else:
        s.lit(x_n)
    if not tight:
        s.lit(1, hdr=3)
    for _ in range(k):
        s.lit(1)
    if e:
        s.lit(1, hdr=2)
    return Case(f"A2_c{cls}_{kind}_S{S}", "A2", s.done(), cls, bytes(s.out),
                claim=dict(S=S, cls=cls, kind=kind, made=made_b, n=x_n))


def _a4(rng, cls: int, d: int) -> Case:
    """A valid stream of exactly STAGE + d bytes: 1-byte literals (two stream
    bytes a byte) and one long literal."""
    slen = STAGE[cls] + d
    want = cls - 8
    h = len(_varint(want))
    k = slen - want - h - 3                     # slen = h + 2 k + 3 + (want - k)
    s = Stream(rng)
    for _ in range(k):
        s.lit(1)
    s.lit(want - k, hdr=3)
    out = s.done()
    assert len(out) == slen
    return Case(f"A4_c{cls}_d{d}", "A4", out, cls, bytes(s.out), claim=dict(slen=slen, cls=cls))


def _cut(c: Case) -> list[Case]:
    """The stream with its last byte cut, and with its tail replaced by 0xFC."""
    return [Case(c.name + "_cut", c.fam, c.s[:-1], c.cap, None, c.osh, c.ish, dict(c.claim, twin=1)),
            Case(c.name + "_fc", c.fam, c.s[:-2] + b"\xfc", c.cap, None, c.osh, c.ish,
                 dict(c.claim, twin=1))]


def _family_a(rng) -> list[Case]:
    cases = []
    for cls, B in CLASSES.items():
        for v, S in enumerate(range(B + A1_RANGE[0], B + A1_RANGE[1] + 1)):
            c = _a1(rng, cls, S, v)
            cases += [c] + _cut(c)
        for kind in A2_KINDS:
            for S in range(B + A2_RANGE[0], B + A2_RANGE[1] + 1):
                cases.append(_a2(rng, cls, S, kind))
        for d in range(-17, 18):
            c = _a4(rng, cls, d)
            cases += [c] + _cut(c)
    return cases


# ---------------------------------------------------------------------------
# Family B
# ---------------------------------------------------------------------------
_FILL = (3000, 40, 61, 700, 64, 65, 10, 5000, 1, 16, 300, 12000)


def _fill_made(s: Stream, target: int) -> Stream:
    """Random literals (short ones and long ones) up to `target` output bytes."""
    k = len(s.body)
    while s.made() < target:
        s.lit(min(target - s.made(), _FILL[k % len(_FILL)]))
        k += 1
    assert s.made() == target
    return s


def _fill_offset(s: Stream, off: int) -> Stream:
    """Literals of at most 60 bytes (they pass through the stream ring, which
    keeps its 2 048-byte refill edges) up to stream offset `off`."""
    gap = off - s.offset()
    assert gap == 0 or gap >= 2, gap
    while gap:
        step = min(gap, 61)
        if gap - step == 1:
            step -= 1
        s.lit(step - 1)
        gap -= step
    assert s.offset() == off
    return s


def _short_tags(s: Stream, nbytes: int) -> Stream:
    """At least nbytes stream bytes of short tags of every form."""
    end = len(s.body) + nbytes
    k = 0
    while len(s.body) < end:
        r = k % 5
        if r == 0:
            s.lit(1 + k % 23)
        elif r == 1:
            s.copy(4 + k % 8, min(1 + k % 200, s.made()), form=1)
        elif r == 2:
            s.copy(1 + k % 64, min(1 + (7 * k) % 3000, s.made()))
        elif r == 3:
            s.lit(60 + k % 5)
        else:
            s.copy(1 + (3 * k) % 64, min(1 + (11 * k) % 900, s.made()), form=3 if k % 3 == 0 else 2)
        k += 1
    return s


def _prev(s: Stream, prev: str) -> int:
    if prev == "lit1":
        s.lit(1)
        return 1
    s.copy(64, 1000)
    return 64


def _b1(rng, dist, form, prev, P, osh, tag) -> Case:
    """Copies of each length at one distance, each right after `prev` (a
    1-byte literal: 63 wild lanes; a 64-byte copy: none).  The first copy is
    made at output position P; the lengths rotate by the case."""
    rot = (FAR_DISTS.index(dist) + form) % 4
    lens = FAR_LENS[rot:] + FAR_LENS[:rot]
    s = Stream(rng)
    _fill_made(s, P - (1 if prev == "lit1" else 64))
    probes = []
    for n in lens:
        pn = _prev(s, prev)
        probes.append(dict(made=s.made(), n=n, dist=dist, kind=form if form == 2 else 4, prev_n=pn))
        s.copy(n, dist, form=form)
    s.lit(50)
    return Case(f"B1_d{dist}_f{form}_{prev}_{tag}", "B1", s.done(), s.made(), bytes(s.out), osh=osh,
                claim=dict(probes=probes, P=P))


def _family_b1(rng) -> list[Case]:
    """Placements 33 000 and 66 000 with every distance, form and prev; the
    wrap placements (made + oshift) & 32767 in -3 .. +3 alternate the form
    with the distance, and take oshift 0, 5, 15 in turn."""
    cases = []
    for di, dist in enumerate(FAR_DISTS):
        for prev in ("lit1", "copy64"):
            for form in (2, 3):
                for P in (33000, 66000):
                    cases.append(_b1(rng, dist, form, prev, P, OSH3[(di + form) % 3], f"P{P}"))
            for k in range(-3, 4):
                osh = OSH3[(k + di) % 3]
                form = 2 if (k + di) % 2 else 3
                P = 32768 + k - osh
                if P < dist:
                    P += 32768
                cases.append(_b1(rng, dist, form, prev, P, osh, f"wrap{k}"))
    return cases


def _family_b2(rng) -> list[Case]:
    cases = []
    s = _fill_made(Stream(rng), 70000)
    s.copy(64, 65536, form=3).lit(3).copy(64, 65537, form=3).lit(1).copy(1, 65536, form=3).lit(9)
    cases.append(Case("B2_65536_65537", "B2", s.done(), s.made(), bytes(s.out), osh=5,
                      claim=dict(dists=[65536, 65537, 65536])))
    for made in (100000, 40000):
        for osh in (5, 15):
            s = _fill_made(Stream(rng), made)
            s.copy(64, made, form=3).copy(64, made, form=3).lit(7).copy(33, made + 100, form=3)
            cases.append(Case(f"B2_dist_is_made{made}_osh{osh}", "B2", s.done(), s.made(),
                              bytes(s.out), osh=osh, claim=dict(dists=[made, made, made + 100],
                                                                first_made=made)))
            s = _fill_made(Stream(rng), made)
            s.raw(bytes([(63 << 2) | 3]) + (made + 1).to_bytes(4, "little")).raw(bytes([8]) + b"abc")
            cases.append(Case(f"B2_dist_made{made}_plus1_osh{osh}", "B2", s.done(want=made + 67),
                              made + 67, None, osh=osh, claim=dict(bad_at=made)))
    return cases


def _family_b3(rng) -> list[Case]:
    """Far copies with nothing between them (runs of 2, 5 and 40), alternating
    with a near copy and a 60-byte literal, until the pattern has made 20 000
    bytes (pending output triggers a flush every 8 KiB)."""
    cases = []
    far = (32705, 32768, 33000, 40000)
    for R in (2, 5, 40):
        for form in (2, 3):
            for start in (33000, 40000):
                s = _fill_made(Stream(rng), 40000 if start == 40000 else 33000)
                k, end, runs = 0, s.made() + 20000, 0
                while s.made() < end:
                    for _ in range(R):
                        d = far[k % 4]
                        s.copy(64 if k % 7 else 33, d if d <= s.made() else s.made(), form=form)
                        k += 1
                    s.copy(64, 1 + k % 500).lit(60)
                    runs += 1
                cases.append(Case(f"B3_run{R}_f{form}_from{start}", "B3", s.done(), s.made(),
                                  bytes(s.out), osh=OSH3[(R + form) % 3], claim=dict(R=R, runs=runs)))
    return cases


def _family_b4(rng) -> list[Case]:
    cases = []
    for want in B4_WANTS:
        for last in ("lit1", "copy64", "litlong"):
            n = dict(lit1=1, copy64=64, litlong=200)[last]
            s = _fill_made(Stream(rng), want - n)
            if last == "copy64":
                s.copy(64, 5000)
            else:
                s.lit(n)
            cases.append(Case(f"B4_want{want}_{last}", "B4", s.done(), want, bytes(s.out),
                              claim=dict(want=want, last_n=n)))
    return cases


def _b5_tags():
    tags = [("copy1", None, 7), ("copy2", None, 33), ("copy4", None, 40)]
    for hdr in (1, 2, 3, 4, 5):
        for n in (1, 60, 61, 64):
            if hdr > 1 or n <= 60:
                tags.append(("lit", hdr, n))
    return tags


def _family_b5(rng) -> list[Case]:
    """One stream per (j, tag): the tag starts at E - j for each of the four
    edges in turn; only literals of at most 60 bytes come before the last
    edge, so the stream ring is refilled at every 2 048."""
    cases = []
    for ti, (kind, hdr, n) in enumerate(_b5_tags()):
        for j in range(7):
            s = Stream(rng, hlen=3).lit(60).lit(60)
            ats = []
            for E in EDGES:
                _fill_offset(s, E - j)
                ats.append(s.offset())
                if kind == "lit":
                    s.lit(n, hdr=hdr)
                else:
                    s.copy(n, 100, form=dict(copy1=1, copy2=2, copy4=3)[kind])
            _short_tags(s, 300)
            _fill_made(s, 17000 + 16 * ti + j)
            cases.append(Case(f"B5_{kind}{'' if hdr is None else f'_h{hdr}'}_n{n}_j{j}", "B5",
                              s.done(), s.made(), bytes(s.out), osh=OSH3[j % 3],
                              ish=ISH3[(ti + j) % 3],
                              claim=dict(ats=ats, kind=kind, hdr=hdr, n=n, j=j)))
    return cases


def _b6(rng, L, follower, res, osh, name) -> Case:
    s = Stream(rng)
    s.lit(60).lit(33).copy(20, 50)
    if follower == "far":
        _fill_made(s, 33000)
    if follower == "end":
        _short_tags(s, 6000)
        _fill_made(s, max(s.made(), 17000 - L))
    if res is not None:
        while (s.made() + osh) & 15 != res:
            s.lit(1)
    at_made = s.made()
    s.lit(L)
    if follower == "copy2":
        s.copy(20, L, form=2 if L < 65536 else 3)
    elif follower == "far":
        d = 32705 + L % 3 if L < 30000 else L + 100
        s.copy(64, d, form=2 if d < 65536 else 3)
    elif follower == "lit60":
        s.lit(60)
    elif follower == "litlong":
        s.lit(100)
    if follower != "end":
        _short_tags(s, 6000)
        _fill_made(s, max(s.made() + 10, 17000))
    return Case(name, "B6", s.done(), s.made(), bytes(s.out), osh=osh,
                claim=dict(L=L, made=at_made, follower=follower, res=res))


def _family_b6(rng) -> list[Case]:
    cases = []
    for li, L in enumerate(B6_LENS):
        for fi, f in enumerate(("copy2", "far", "lit60", "litlong", "end")):
            cases.append(_b6(rng, L, f, None, OSH3[(li + fi) % 3], f"B6_L{L}_{f}"))
    for L in B6_RESIDUE_LENS:
        for res in range(16):
            osh = OSH3[res % 3]
            cases.append(_b6(rng, L, "lit60", res, osh, f"B6_L{L}_res{res}"))
    return cases


def _family_b7(rng) -> list[Case]:
    """A long literal whose end offset x + nb is M + d; its tag starts 150
    bytes below M - 2 048 ("below") or 300 bytes above it ("above")."""
    cases = []
    for M in B7_M:
        for where in ("below", "above"):
            for d in range(-20, 21):
                T = M - 2048 - 150 if where == "below" else M - 2048 + 300
                s = Stream(rng, hlen=3).lit(60)
                _fill_offset(s, T)
                L = M + d - T - 3
                s.lit(L, hdr=3)
                end = s.offset()
                _short_tags(s, 3000)
                _fill_made(s, max(s.made() + 10, 17000 + d))
                cases.append(Case(f"B7_M{M}_{where}_d{d}", "B7", s.done(), s.made(), bytes(s.out),
                                  osh=OSH3[d % 3], ish=ISH3[(d // 3) % 3],
                                  claim=dict(M=M, d=d, where=where, at=T, end=end)))
    return cases


def _family_b8(rng) -> list[Case]:
    """A 64-byte overlapping copy made at (made + oshift) & 32767 = 32768 - 70
    + i, i in 0 .. 76; three of the nine distances at each position, in
    rotation, so each distance stands at 25 or 26 positions spread over the
    range."""
    cases = []
    for i in range(77):
        for r in range(3):
            dist = B8_DISTS[(i + 3 * r) % 9]
            osh = OSH3[(i + r) % 3]
            made = 32768 - 70 + i - osh
            s = _fill_made(Stream(rng), made)
            s.copy(64, dist).lit(30).copy(64, dist).lit(11)
            cases.append(Case(f"B8_pos{i - 70}_d{dist}", "B8", s.done(), s.made(), bytes(s.out),
                              osh=osh, claim=dict(made=made, dist=dist, pos=(32768 - 70 + i) & 32767)))
    return cases


def _family_b9(rng) -> list[Case]:
    """Every reject after the output ring has wrapped."""
    def base():
        s = _fill_made(Stream(rng), 40500)
        _short_tags(s, 400)
        return s
    cases = []
    k = [0]

    def add(name, s: Stream, want: int, cap: int | None = None):
        cases.append(Case("B9_" + name, "B9", s.done(want=want), want if cap is None else cap, None,
                          osh=OSH3[k[0] % 3], ish=ISH3[(k[0] // 3) % 3],
                          claim=dict(made=s.made())))
        k[0] += 1

    bad_tags = [
        ("dist0", bytes([2, 0, 0])),
        ("dist0_copy4", bytes([3, 0, 0, 0, 0])),
        ("dist_2p31", bytes([(63 << 2) | 3]) + (2**31).to_bytes(4, "little")),
        ("lit_2p31", bytes([63 << 2]) + b"\xff\xff\xff\x7f"),
        ("header_past_stream", bytes([62 << 2, 0xff, 0xff])),
        ("length_bytes_cut", bytes([61 << 2, 0x10])),
        ("lit_past_stream", bytes([20 << 2]) + b"short"),
        ("copy1_cut", bytes([1])),
        ("copy2_cut", bytes([2, 1])),
        ("copy4_cut", bytes([3, 1, 0, 0])),
    ]
    for name, bad in bad_tags:
        s = base()
        add(name, s.raw(bad), s.made() + 70)
    s = base()
    made = s.made()
    add("dist_made_plus1", s.raw(bytes([(63 << 2) | 3]) + (made + 1).to_bytes(4, "little")), made + 64)
    for name, keep in (("head", 5), ("body", 2500), ("tail", 4995)):
        s = base()
        made = s.made()
        add("long_lit_cut_" + name, s.raw(_lit_header(5000) + rng.randbytes(keep)), made + 5000)
    for name, dw in (("want_minus1", -1), ("want_plus1", 1)):
        for last in ("lit", "copy"):
            s = base()
            if last == "lit":
                s.lit(300)
            else:
                s.copy(64, 33000)
            add(f"{name}_{last}", s, s.made() + dw, s.made() + 16)
    return cases


# ---------------------------------------------------------------------------
# Family C: the two blocks at the pair decoder's limit
# ---------------------------------------------------------------------------
def _huge(rng, want: int) -> tuple[bytes, bytes]:
    """One literal, then 64-byte copies at dist 1 (built without the op-by-op
    walk: the output is the literal and a run of its last byte)."""
    lit = rng.randbytes(1000)
    n, rem = divmod(want - 1000, 64)
    body = _lit_header(1000) + lit + bytes([(63 << 2) | 2, 1, 0]) * n
    if rem:
        body += bytes([((rem - 1) << 2) | 2, 1, 0])
    return _varint(want) + body, lit + lit[-1:] * (want - 1000)


def _family_c(rng) -> list[Case]:
    cases = []
    for want in (0xffffff, 0x1000000):
        s, out = _huge(rng, want)
        cases.append(Case(f"C_want{want:#x}", "C", s, want, out, claim=dict(want=want)))
        cases.append(Case(f"C_want{want:#x}_cut", "C", s[:-1], want, None, claim=dict(want=want)))
    return cases


_CASES = None


def _cases() -> list[Case]:
    global _CASES
    if _CASES is None:
        rng = random.Random(20262)
        _CASES = (_family_a(rng) + _family_b1(rng) + _family_b2(rng) + _family_b3(rng) +
                  _family_b4(rng) + _family_b5(rng) + _family_b6(rng) + _family_b7(rng) +
                  _family_b8(rng) + _family_b9(rng) + _family_c(rng))
    return _CASES


def _fam(*fams) -> list[Case]:
    return [c for c in _cases() if c.fam in fams]


_REF: dict[str, bytes | None] = {}


def _expected(c: Case):
    """The reference's decode of the case's stream (None: it rejects it)."""
    if c.name not in _REF:
        _REF[c.name] = oracle.best().decode(c.s)
    return _REF[c.name]


B_FAMS = ("B1", "B2", "B3", "B4", "B5", "B6", "B7", "B8", "B9")


# ---------------------------------------------------------------------------
# The CPU test
# ---------------------------------------------------------------------------
def _find(ops, **kw):
    return [op for op in ops if all(op[k] == v for k, v in kw.items())]


def test_cases_are_what_they_say():
    cases = _cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert sum(len(c.s) for c in cases) < 40_000_000

    # every valid stream is the reference's too, every reject is rejected
    for c in cases:
        exp = _expected(c)
        if c.out is None:
            assert exp is None, c.name
        else:
            assert exp == c.out and len(c.out) <= c.cap and _header(c.s) == len(c.out), c.name

    # ---- A: S recomputed from the bytes; the ranges complete
    seen = {(f, cls): set() for f in ("A1", "A2") for cls in CLASSES}
    kinds = {(cls, k): set() for cls in CLASSES for k in A2_KINDS}
    excess = {(cls, k): set() for cls in CLASSES for k in A2_KINDS + ("A1",)}
    for c in _fam("A1", "A2"):
        if c.out is None:
            continue
        S, at = run_ahead(c.s)
        tight = c.fam == "A2" and c.claim["kind"].endswith("_lit")
        assert S == c.claim["S"] and len(at) == (2 if tight else 1), (c.name, S)
        op = at[0]
        if tight:                        # X, and the plain 1-byte literal right after it
            assert at[1]["at"] == op["end"] and (at[1]["kind"], at[1]["n"], at[1]["lm"]) == (
                0, 1, at[1]["at"] + 1), c.name
        seen[(c.fam, c.claim["cls"])].add(S)
        cls = c.claim["cls"]
        excess[(cls, c.claim.get("kind", "A1"))].add(S - CLASSES[cls] + ((STAGE[cls] - len(c.s)) & 15))
        if c.fam == "A1":
            assert op["kind"] == 0 and op["n"] == 1                      # the first 1-byte literal
            _, ops, clean = walk(c.s)
            assert clean and ops[0]["n"] == 4 and all(
                o["kind"] == 2 and o["n"] == 64 and o["dist"] == 4 for o in ops[1:ops.index(op) - 1])
            last = ops[ops.index(op) - 1]
            assert last["kind"] == 2 and 49 <= last["n"] <= 64 and last["dist"] == 4
        else:
            k = c.claim["kind"]
            assert op["made"] == c.claim["made"] and op["n"] == c.claim["n"], c.name
            hdr = op["lm"] - op["at"]
            assert dict(copy2=op["kind"] == 2 and op["dist"] >= op["n"],
                        copy4=op["kind"] == 4,
                        copy2_lit=op["kind"] == 2 and op["dist"] >= op["n"],
                        copy4_lit=op["kind"] == 4,
                        overlap=op["kind"] in (1, 2) and op["dist"] < op["n"],
                        lit60=op["kind"] == 0 and op["n"] <= 60 and hdr == 1,
                        lit61_64=op["kind"] == 0 and 61 <= op["n"] <= 64,
                        litlong=op["kind"] == 0 and op["n"] > 64)[k], c.name
            kinds[(c.claim["cls"], k)].add(S)
    for cls, B in CLASSES.items():
        assert seen[("A1", cls)] == set(range(B + A1_RANGE[0], B + A1_RANGE[1] + 1)), cls
        # the excess over the bound at sh = oshift = 0, which is what decides
        assert excess[(cls, "A1")] >= set(range(A1_RANGE[0] + 15, A1_RANGE[1] + 1)), cls
        for k in A2_KINDS:
            assert excess[(cls, k)] >= set(range(A2_RANGE[0] + 15, A2_RANGE[1] + 1)), (cls, k)
        for k in A2_KINDS:
            assert kinds[(cls, k)] == set(range(B + A2_RANGE[0], B + A2_RANGE[1] + 1)), (cls, k)
        lens = {len(c.s) for c in _fam("A4") if c.out is not None and c.claim["cls"] == cls}
        assert lens == set(range(STAGE[cls] - 17, STAGE[cls] + 18)), cls
    a1 = {c.name for c in _fam("A1")}
    assert all(n + "_cut" in a1 and n + "_fc" in a1 for n in a1 if not n.endswith(("_cut", "_fc")))
    assert len([c for c in _a3_cases(4608) if c.fam == "A1"]) == 3 * (A3_RANGE[1] - A3_RANGE[0] + 1)

    # ---- B1: each probe is in the stream, right after its prev op, at its place
    got, wrap = set(), set()
    for c in _fam("B1"):
        _, ops, clean = walk(c.s)
        probes = c.claim["probes"]
        assert clean and probes[0]["made"] == c.claim["P"] and c.osh in OSH3, c.name
        for p in probes:
            (op,) = _find(ops, made=p["made"], n=p["n"], dist=p["dist"], kind=p["kind"])
            before = ops[ops.index(op) - 1]
            assert before["n"] == p["prev_n"] and before["kind"] == (0 if p["prev_n"] == 1 else 2)
            assert before["made"] + before["n"] == op["made"]
            if "wrap" not in c.name:
                got.add((p["dist"], p["n"], p["kind"], p["prev_n"], c.claim["P"]))
        if "wrap" in c.name:
            k = (probes[0]["made"] + c.osh + 3) % 32768 - 3
            wrap.add((probes[0]["dist"], probes[0]["prev_n"], k, probes[0]["kind"]))
    assert got == {(d, n, kind, pn, P) for d in FAR_DISTS for n in FAR_LENS for kind in (2, 4)
                   for pn in (1, 64) for P in (33000, 66000)}
    for d in FAR_DISTS:
        for pn in (1, 64):
            assert {k for (dd, p, k, _) in wrap if (dd, p) == (d, pn)} == set(range(-3, 4)), d
            assert {kind for (dd, p, _, kind) in wrap if (dd, p) == (d, pn)} == {2, 4}, d

    # ---- B2 .. B4
    for c in _fam("B2"):
        _, ops, clean = walk(c.s)
        if c.out is not None:
            assert clean and [o["dist"] for o in ops if o["kind"] == 4] == c.claim["dists"], c.name
            if "first_made" in c.claim:
                (op,) = _find(ops, made=c.claim["first_made"], kind=4)
                assert op["dist"] == op["made"] and c.osh != 0
        else:
            assert not clean and sum(o["n"] for o in ops) == c.claim["bad_at"], c.name
            bad = c.s[ops[-1]["end"]:]
            assert bad[0] & 3 == 3 and int.from_bytes(bad[1:5], "little") == c.claim["bad_at"] + 1
    assert {c.claim["R"] for c in _fam("B3")} == {2, 5, 40}
    for c in _fam("B3"):
        _, ops, clean = walk(c.s)
        far = [o["kind"] != 0 and o["dist"] > 32704 for o in ops]
        runs = [len(r) for r in "".join("f" if f else "." for f in far).split(".") if r]
        assert clean and runs.count(c.claim["R"]) >= c.claim["runs"] - 1, c.name
        first = ops[far.index(True)]["made"]
        assert ops[-1]["made"] - first >= 2 * 8192                         # several flushes inside
    wants = set()
    for c in _fam("B4"):
        want, ops, clean = walk(c.s)
        assert clean and want == c.claim["want"] == c.cap and ops[-1]["n"] == c.claim["last_n"]
        wants.add((want, ops[-1]["n"]))
    assert wants == {(w, n) for w in B4_WANTS for n in (1, 64, 200)}

    # ---- B5: a tag of the stated form at E - j for every E, j and form
    got = set()
    for c in _fam("B5"):
        _, ops, clean = walk(c.s)
        assert clean and c.claim["ats"] == [E - c.claim["j"] for E in EDGES], c.name
        for E, at in zip(EDGES, c.claim["ats"]):
            (op,) = _find(ops, at=at)
            kind = {0: "lit", 1: "copy1", 2: "copy2", 4: "copy4"}[op["kind"]]
            hdr = op["lm"] - op["at"] if kind == "lit" else None
            assert (kind, hdr, op["n"]) == (c.claim["kind"], c.claim["hdr"], c.claim["n"]), c.name
            if kind == "lit" and op["n"] >= 60 and c.claim["j"] >= 1:
                assert op["at"] < E < op["end"]                           # its bytes cross E
            # nothing before the last edge bypasses the stream ring
            assert all(o["n"] <= 64 for o in ops if o["at"] <= at)
            got.add((E, c.claim["j"], kind, hdr, op["n"]))
        assert c.ish in ISH3
    assert got == {(E, j, k, h, n) for E in EDGES for j in range(7) for (k, h, n) in _b5_tags()}
    assert ("lit", 5, 64) in _b5_tags() and ("lit", 1, 60) in _b5_tags() and len(_b5_tags()) == 21
    assert {(c.claim["kind"], c.claim["hdr"], c.claim["n"], c.ish) for c in _fam("B5")} >= {
        (k, h, n, i) for (k, h, n) in _b5_tags() for i in ISH3}

    # ---- B6, B7, B8
    got, res = set(), set()
    for c in _fam("B6"):
        _, ops, clean = walk(c.s)
        (op,) = _find(ops, made=c.claim["made"], n=c.claim["L"], kind=0)
        nxt = ops[ops.index(op) + 1] if op is not ops[-1] else None
        f = c.claim["follower"]
        assert clean and dict(
            copy2=lambda: nxt["kind"] in (2, 4) and nxt["dist"] == op["n"],
            far=lambda: nxt["kind"] in (2, 4) and nxt["dist"] > 32704,
            lit60=lambda: nxt["kind"] == 0 and nxt["n"] == 60,
            litlong=lambda: nxt["kind"] == 0 and nxt["n"] > 64,
            end=lambda: nxt is None)[f](), c.name
        if f == "end":
            assert sum(o["end"] - o["at"] for o in ops if o["n"] <= 64) >= 6000
        else:
            assert sum(o["end"] - o["at"] for o in ops[ops.index(op) + 2:] if o["n"] <= 64) >= 6000
        if c.claim["res"] is None:
            got.add((op["n"], f))
        else:
            assert (op["made"] + c.osh) & 15 == c.claim["res"]
            res.add((op["n"], c.claim["res"]))
    assert got == {(L, f) for L in B6_LENS for f in ("copy2", "far", "lit60", "litlong", "end")}
    assert res == {(L, r) for L in B6_RESIDUE_LENS for r in range(16)}
    got = set()
    for c in _fam("B7"):
        _, ops, clean = walk(c.s)
        (op,) = _find(ops, at=c.claim["at"])
        M = c.claim["M"]
        assert clean and op["kind"] == 0 and op["n"] > 64 and op["end"] == M + c.claim["d"], c.name
        assert (op["at"] < M - 2048) == (c.claim["where"] == "below")
        assert all(o["n"] <= 64 for o in ops if o["at"] < op["at"])
        got.add((M, c.claim["where"], op["end"] - M))
    assert got == {(M, w, d) for M in B7_M for w in ("below", "above") for d in range(-20, 21)}
    got = set()
    for c in _fam("B8"):
        _, ops, clean = walk(c.s)
        (op,) = _find(ops, made=c.claim["made"])
        assert clean and op["n"] == 64 and op["dist"] == c.claim["dist"] < 64, c.name
        got.add(((op["made"] + c.osh + 70) % 32768 - 70, op["dist"]))
    assert {p for p, _ in got} == set(range(-70, 7))
    for d in B8_DISTS:
        ps = sorted(p for p, dd in got if dd == d)
        assert len(ps) >= 25 and ps[0] <= -62 and ps[-1] >= -2 and max(
            b - a for a, b in zip(ps, ps[1:])) <= 3, d

    # ---- B9, C
    for c in _fam("B9"):
        assert c.claim["made"] > 40000 and _header(c.s) is not None and _header(c.s) <= c.cap, c.name
    assert len(_fam("B9")) >= 18
    for c in _fam("C"):
        assert _header(c.s) == c.claim["want"]
    # outputs of the B cases are in the wide decoder's range
    for c in _fam(*B_FAMS):
        assert 16896 < c.cap <= 140000, c.name


# ---------------------------------------------------------------------------
# Routes
# ---------------------------------------------------------------------------
def _verdict(gpu, c: Case, code: int, got: bytes | None) -> bool:
    exp = _expected(c)
    h = _header(c.s)
    if h is not None and h > c.cap:
        return code == gpu.LGS_ST_NOSPACE
    if exp is None:
        return code == gpu.LGS_ST_CORRUPT
    return code == gpu.LGS_ST_OK and got == exp


def _report(bad: list[str]):
    assert not bad, f"{len(bad)} differ from the reference: " + " ".join(bad[:400])


def _host(gpu, cases: list[Case], cap: int | None = None, chunk: int = 400) -> list[str]:
    """Host batches of under 512 blocks; the names that differ."""
    bad = []
    for a in range(0, len(cases), chunk):
        part = cases[a:a + chunk]
        res, st = gpu.decode_batch_host([c.s for c in part], [cap or c.cap for c in part])
        bad += [c.name + ":host" for c, o, code in zip(part, res, st) if not _verdict(gpu, c, int(code), o)]
    return bad


def _device(gpu, cases: list[Case], shifts=None, max_cap: int | None = None, packed: int | None = None,
            tag: str = "dev") -> list[str]:
    """One device batch with explicit offsets.  shifts: (ish, oshift) per case
    (the case's own by default).  Guarded layout: 32 bytes of 0xEE before each
    output and at least 32 after its capacity, which must come back unchanged.
    packed=k: outputs back to back, the first at 32 + k, guards at both ends."""
    import torch
    n = len(cases)
    shifts = shifts or [(c.ish, c.osh) for c in cases]
    in_off, out_off, p, q = [], [], 0, 0
    for c, (ish, osh) in zip(cases, shifts):
        in_off.append(p + ish)
        p = (p + ish + len(c.s) + 31) & ~15
        if packed is None:
            out_off.append(q + 32 + osh)
            q = (q + 32 + osh + c.cap + 47) & ~15
    if packed is not None:
        q = 32 + packed
        for c in cases:
            out_off.append(q)
            q += c.cap
        q = (q + 63) & ~15
    buf = np.zeros(p + 64, dtype=np.uint8)
    for c, o in zip(cases, in_off):
        buf[o:o + len(c.s)] = np.frombuffer(c.s, dtype=np.uint8)
    dev = "cuda"
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    d_in = torch.from_numpy(buf).to(dev)
    d_out = torch.full((q + 64,), 0xEE, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    gpu.decode_batch(d_in, i64(in_off), i32([len(c.s) for c in cases]), d_out, i64(out_off),
                     i32([c.cap for c in cases]), d_len, d_st, max_cap or max(c.cap for c in cases))
    torch.cuda.synchronize()
    out, olen, st = d_out.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy()
    bad = []
    for k, (c, o) in enumerate(zip(cases, out_off)):
        code = int(st[k])
        got = out[o:o + int(olen[k])].tobytes() if code == gpu.LGS_ST_OK else None
        if not _verdict(gpu, c, code, got):
            bad.append(f"{c.name}:{tag}")
        elif packed is None:
            end = out_off[k + 1] - 32 - shifts[k + 1][1] if k + 1 < n else len(out)
            if not ((out[o - 32 - shifts[k][1]:o] == 0xEE).all() and (out[o + c.cap:end] == 0xEE).all()):
                bad.append(f"{c.name}:{tag}:guard")
    if packed is not None:
        if not ((out[:out_off[0]] == 0xEE).all() and (out[out_off[-1] + cases[-1].cap:] == 0xEE).all()):
            bad.append(f"{tag}:guard")
    return bad


def _dropin(gpu, cases: list[Case]) -> list[str]:
    return [c.name + ":dropin" for c in cases if gpu.decode(c.s) != _expected(c)]


def _mixed(cases: list[Case], every: int = 3) -> list[Case]:
    """Rejects beside valid neighbours: the cases as they come, a valid B4
    block after every `every` of them."""
    pad = [c for c in _fam("B4") if c.cap < 30000]
    res = []
    for k, c in enumerate(cases):
        res.append(c)
        if k % every == every - 1:
            res.append(pad[(k // every) % len(pad)])
    return res


# ---------------------------------------------------------------------------
# A on the GPU
# ---------------------------------------------------------------------------
def _a3_cases(cls: int) -> list[Case]:
    B = CLASSES[cls]
    return [c for c in _fam("A1", "A2") if c.cap == cls and
            B + A3_RANGE[0] <= c.claim["S"] <= B + A3_RANGE[1] and
            c.claim.get("kind", "copy2_lit").endswith("_lit")]


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("fam", ["A1", "A2", "A4"])
def test_wave_in_place_bound_host(gpu, force, cls, fam):
    force("decoder", "wave")
    cases = [c for c in _fam(fam) if c.cap == cls]
    assert len(cases) >= 100
    _report(_host(gpu, cases, chunk=500))


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(CLASSES))
def test_wave_in_place_bound_alignments(gpu, force, cls):
    # A3: valid streams and their rejected twins side by side at each
    # (sh, oshift); the guard bytes around every output come back unchanged.
    force("decoder", "wave")
    cases = _a3_cases(cls)
    bad = []
    for sh in (0, 1, 7, 15):
        for osh in (0, 1, 7, 15):
            bad += _device(gpu, cases, shifts=[(sh, osh)] * len(cases), max_cap=cls,
                           tag=f"sh{sh}:osh{osh}")
    _report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(CLASSES))
def test_wave_staging_limit_alignments(gpu, force, cls):
    force("decoder", "wave")
    cases = [c for c in _fam("A4") if c.cap == cls]
    bad = []
    for sh, osh in ((0, 0), (1, 15), (15, 1), (7, 7)):
        bad += _device(gpu, cases, shifts=[(sh, osh)] * len(cases), max_cap=cls,
                       tag=f"sh{sh}:osh{osh}")
    _report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("service", ["1", "0"])
def test_wave_in_place_bound_dropin(gpu, force, service):
    # A5: the service waves (decode_item<4608>), and the one-item launch
    force("service", service)
    _report(_dropin(gpu, _a3_cases(4608)))


# ---------------------------------------------------------------------------
# B on the GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fam", B_FAMS)
def test_wide_rings_host(gpu, fam):
    cases = _fam(fam)
    _report(_host(gpu, _mixed(cases) if fam in ("B2", "B9") else cases))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", B_FAMS)
def test_wide_rings_device(gpu, fam):
    cases = _fam(fam)
    if fam in ("B2", "B9"):
        cases = _mixed(cases)
    bad = []
    for a in range(0, len(cases), 300):
        bad += _device(gpu, cases[a:a + 300])
    if fam == "B5":                     # each stream at each input alignment
        for ish in ISH3:
            bad += _device(gpu, cases, shifts=[(ish, c.osh) for c in cases], tag=f"ish{ish}")
    if fam in ("B1", "B2"):             # each stream at each of the three output alignments
        for osh in OSH3:
            part = [c for c in cases if "wrap" not in c.name]
            bad += _device(gpu, part, shifts=[(c.ish, osh) for c in part], tag=f"osh{osh}")
    _report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("osh", range(16))
def test_wide_block_ends_every_alignment(gpu, osh):
    # B4: guarded at this oshift, and packed back to back with no slack
    # (block k then starts where block k - 1 ends; sixteen starts give every
    # block every alignment).
    cases = _fam("B4")
    bad = _device(gpu, cases, shifts=[(0, osh)] * len(cases), tag=f"osh{osh}")
    bad += _device(gpu, cases, packed=osh, tag=f"packed{osh}")
    bad += _device(gpu, _mixed(_fam("B9"), 1), packed=osh, tag=f"packed{osh}")
    _report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", B_FAMS)
def test_wide_rings_dropin(gpu, fam):
    cases = [c for c in _fam(fam) if DROPIN_MIN <= (_header(c.s) or 0) <= DROPIN_MAX]
    assert cases
    _report(_dropin(gpu, cases))


@pytest.mark.gpu
def test_wide_rings_from_the_split(gpu):
    # A batch of at least 512 blocks with 4 KiB and 16 KiB blocks between
    # them: the wide kernel runs from the split's index list and count.
    small = [c for c in _fam("A1", "A2")]
    cases = []
    for k, c in enumerate(_fam(*B_FAMS)):
        cases += [c, small[k % len(small)]]
    assert len(cases) >= 512
    bad = []
    for a in range(0, len(cases), 1200):
        part = cases[a:a + 1200]
        if len(part) < 512:
            part = cases[-512:]
        bad += _host(gpu, part, chunk=len(part))
    _report(bad)


def _with_probe(kernels, probe_kernels):
    return list(kernels) + [pytest.param(k, marks=pytest.mark.probe) for k in probe_kernels if PROBE]


# ---------------------------------------------------------------------------
# C: the pair decoder above 4 608 bytes
# ---------------------------------------------------------------------------
def _c_pool() -> list[Case]:
    return _mixed(_fam("B1", "B2", "B3", "B6", "B9"), 5)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 65, 130])
def test_pair_decoder_large_outputs(gpu, force, count):
    force("decoder", "ring")
    pool = _c_pool()
    if count == 1:                      # one of each family and every 23rd: one-block launches
        pool = pool[::23]
    bad = _host(gpu, pool, chunk=count)
    if count == 65:
        for a in range(0, len(pool), 390):
            bad += _device(gpu, pool[a:a + 65], tag="ring")
    _report(bad)


@pytest.mark.gpu
def test_pair_decoder_limit(gpu, force):
    # want = 0xffffff stays in the pair kernel, 0x1000000 goes by its size
    # class; both the reference's bytes, their truncated twins corrupt.
    force("decoder", "ring")
    cases = _fam("C")
    for c in cases:
        t0 = time.perf_counter()
        bad = _host(gpu, [c])
        print(f"{c.name}: {time.perf_counter() - t0:.3f} s")
        _report(bad)
    _report(_host(gpu, cases + _fam("B4")[:3]))
