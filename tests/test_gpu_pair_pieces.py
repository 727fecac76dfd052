"""The pair decoder's pieces, flush jobs and refills, case by case
(decode_pair_kernel): every chunk count of a piece, every copy
distance class, every position of a piece in the 256-byte output ring against
every alignment of the destination, literals across the input ring's wrap,
overlapping copies beside plain ones, flush jobs of every size and blocks
that all refill in one trip.

Streams are built op by op.  All blocks of a batch share the number of ops
before the piece under test, so the mover meets the pieces of one batch in the
same slot of the same trip and the lanes of its wave carry different cases.
Every batch goes through the "ring" route and is compared with the reference
decoder exactly: status, length, bytes, and nothing written outside the block.
"""
from __future__ import annotations

import random

import numpy as np
import pytest

import oracle
from test_gpu_decode_pair import CAP, Stream

pytestmark = pytest.mark.gpu

PIECES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
POSITIONS = (0, 1, 47, 48, 63, 64, 177, 192, 193, 240, 241, 255)
ALIGNS = (0, 1, 8, 15)
K_PREFIX = 9                       # ops before the piece under test
STRIDE_OUT = CAP + 256             # a multiple of 128: dst & 127 is the case's own


def _prefix(s: Stream, total: int, k: int = K_PREFIX) -> Stream:
    """`total` output bytes as exactly k literals of <= 60 bytes."""
    assert k <= total <= 60 * k
    for j in range(k):
        s.lit(total // k + (1 if j < total % k else 0))
    return s


def _tail(s: Stream) -> Stream:
    # What follows the piece reads it back: a near copy over the piece's end
    # and a literal (they overwrite whatever a 16-byte write left past it).
    return s.copy(min(20, len(s.out)), min(24, len(s.out))).lit(5)


def _piece(s: Stream, kind: str, n: int, d: int = 0) -> Stream:
    return s.lit(n) if kind == "lit" else s.copy(n, d)


def _at(rng, made: int, kind: str, n: int, d: int = 0) -> bytes:
    """One piece that starts at output position 256 + made (made mod 256 in
    the ring; 256 bytes of history: every near distance is valid)."""
    s = _prefix(Stream(rng), 256 + made)
    return _tail(_piece(s, kind, n, d)).done()


def _pad_stream_to(s: Stream, pos: int, header: int = 2) -> Stream:
    """Literals until the next tag starts at stream offset pos (mod 192)."""
    gap = (pos - (s.pos() + header)) % 192
    if gap < 2:
        gap += 192
    while gap:                     # a literal of n bytes takes n + 1 stream bytes
        step = min(gap, 61)
        if gap - step == 1:
            step -= 1
        s.lit(step - 1)
        gap -= step
    assert (s.pos() + header) % 192 == pos % 192
    return s


_REF: dict[bytes, bytes] = {}


def _run(gpu, cases) -> None:
    """cases: (stream, dst & 127).  One launch; every block exact."""
    import torch
    assert 64 <= len(cases) <= 256
    streams = [c[0] for c in cases]
    n = len(streams)
    lens = np.array([len(s) for s in streams], dtype=np.uint32)
    stride_in = (int(lens.max()) + 31) & ~15
    buf = np.zeros(n * stride_in + 64, dtype=np.uint8)
    in_off = np.arange(n, dtype=np.uint64) * np.uint64(stride_in)
    for s, o in zip(streams, in_off):
        buf[int(o):int(o) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    out_off = (np.arange(n, dtype=np.uint64) * np.uint64(STRIDE_OUT) + np.uint64(128) +
               np.array([c[1] for c in cases], dtype=np.uint64))
    dev = "cuda"
    d_out = torch.full((n * STRIDE_OUT + 512,), 0xEE, dtype=torch.uint8, device=dev)
    assert d_out.data_ptr() % 128 == 0
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu.decode_batch(torch.from_numpy(buf).to(dev),
                     torch.from_numpy(in_off.view(np.int64)).to(dev),
                     torch.from_numpy(lens.view(np.int32)).to(dev), d_out,
                     torch.from_numpy(out_off.view(np.int64)).to(dev),
                     torch.full((n,), CAP, dtype=torch.int32, device=dev), d_len, d_st, CAP)
    torch.cuda.synchronize()
    out, olen, st = d_out.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy()
    end = 0
    for k, s in enumerate(streams):
        if s not in _REF:
            _REF[s] = oracle.best().decode(s)
        exp = _REF[s]
        assert exp is not None and len(exp) <= CAP, k
        o = int(out_off[k])
        assert st[k] == gpu.LGS_ST_OK and int(olen[k]) == len(exp), (k, cases[k][1])
        got = out[o:o + len(exp)].tobytes()
        if got != exp:
            at = next(j for j in range(len(exp)) if got[j] != exp[j])
            raise AssertionError((k, cases[k][1], "first wrong byte", at, "of", len(exp)))
        assert (out[end:o] == 0xEE).all(), k            # between the blocks: untouched
        end = o + len(exp)
    assert (out[end:] == 0xEE).all()


def _fill(cases, n: int = 64):
    """At least n blocks (a whole wave of different cases), at most 256."""
    res = list(cases)
    k = 0
    while len(res) < n:
        res.append(cases[k % len(cases)])
        k += 1
    assert len(res) <= 256
    return res


def _spread(k: int) -> int:
    # a destination offset mod 128 for cases that do not choose one
    return (37 * k) % 128


def test_piece_lengths(gpu, force):
    # 1-64 bytes: one to four chunks, each as a literal and as a copy that
    # does not overlap, all at one ring position; then at another.
    force("decoder", "ring")
    rng = random.Random(301)
    for made in (44, 250):
        cases = []
        for n in PIECES:
            cases.append(_at(rng, made, "lit", n))
            cases.append(_at(rng, made, "copy", n, 100))
            cases.append(_at(rng, made, "copy", n, n))
        assert len(cases) == 36
        _run(gpu, _fill([(s, _spread(k)) for k, s in enumerate(cases)]))


def test_copy_distances(gpu, force):
    # dist = piece, piece + 1, and the distances whose source lies in ring
    # slots that the piece's own later chunks overwrite (191-240); 241 is the
    # far path.
    force("decoder", "ring")
    rng = random.Random(302)
    for made in (7, 200):
        cases = []
        for n in (17, 33, 49, 64):
            for d in (n, n + 1, 64, 65, 128, 191, 192, 193, 239, 240, 241):
                if d >= n:
                    cases.append(_at(rng, made, "copy", n, d))
        assert 40 <= len(cases) <= 44
        _run(gpu, _fill([(s, _spread(k)) for k, s in enumerate(cases)]))


@pytest.mark.parametrize("variant", range(3))
def test_ring_positions_and_alignments(gpu, force, variant):
    # made mod 256 at the piece's start x dst & 15: the mirror write
    # (r < 64), the wrapped write (r > 240) and reads that run into the
    # mirror, at every shift of the ring.
    force("decoder", "ring")
    rng = random.Random(303 + variant)
    kinds = (("lit", 64, 0), ("copy", 64, 64), ("copy", 49, 239), ("copy", 33, 100),
             ("lit", 17, 0), ("copy", 64, 240), ("copy", 48, 192), ("lit", 49, 0))
    cases = []
    for i, made in enumerate(POSITIONS):
        for j, a in enumerate(ALIGNS):
            kind, n, d = kinds[(3 * i + j + variant * 3) % len(kinds)]
            # (the block's first line is 16 to 128 bytes long)
            cases.append((_at(rng, made, kind, n, d), a + 16 * ((i + j) % 8)))
    assert len(cases) == 48
    _run(gpu, _fill(cases))


def test_literal_wraps_input_ring(gpu, force):
    # A 64-byte literal whose bytes start 16k + j below the input ring's end:
    # the wrap falls inside chunk k (j = 1, 8, 15) or at its start (j = 16).
    force("decoder", "ring")
    rng = random.Random(304)
    cases = []
    for k in range(4):
        for j in (1, 8, 15, 16):
            lo = 192 - 16 * k - j
            s = Stream(rng).lit(60).lit(60).lit(20)
            for n in (64, 61):                      # two laps of the ring
                _pad_stream_to(s, lo - 2)            # (the literal's tag: two bytes)
                s.lit(n)
                s.copy(30, 40)
            cases.append(_tail(s).done())
    assert len(cases) == 16
    _run(gpu, _fill([(s, _spread(k)) for k, s in enumerate(cases)]))


def test_overlapping_copies_beside_plain(gpu, force):
    # Pattern copies (dist 1, 2, 4, 8) and serial ones (3, 5, 7, 12, 15) in
    # even lanes, plain pieces in odd lanes.
    force("decoder", "ring")
    rng = random.Random(305)
    for made in (60, 245):
        cases = []
        for d in (1, 2, 4, 8, 3, 5, 7, 12, 15):
            for n in (d + 1, 17, 33, 50, 64):
                cases.append(_at(rng, made, "copy", n, d))
                plain = PIECES[len(cases) % len(PIECES)]
                cases.append(_at(rng, made, "lit", plain) if len(cases) % 4 == 1
                             else _at(rng, made, "copy", plain, 70 + len(cases)))
        assert len(cases) == 90
        _run(gpu, [(s, _spread(k)) for k, s in enumerate(cases)])


def _block_of(rng, want: int) -> bytes:
    # `want` output bytes in literals and non-overlapping copies of <= 64
    s = Stream(rng)
    k = 0
    while len(s.out) < want:
        n = min(want - len(s.out), (64, 23, 64, 5, 40)[k % 5])
        if k % 2 and len(s.out) >= 2 * n:
            s.copy(n, 2 * n if 2 * n <= 240 else n)
        else:
            while n > 60:
                s.lit(30)
                n -= 30
            s.lit(n)
        k += 1
    assert len(s.out) == want
    return s.done()


def test_flush_job_sizes(gpu, force):
    # First-line jobs of 1, 15, 16, 17, 112, 127 and 128 bytes (dst & 127),
    # tails of the same sizes, interior lines between them, blocks that end
    # on a line, blocks inside one line and blocks of less than 128 bytes
    # that cross one.
    force("decoder", "ring")
    rng = random.Random(306)
    sizes = (1, 15, 16, 17, 112, 127, 128)
    cases = []
    for first in sizes:
        for tail in sizes:
            a = (128 - first) % 128
            for lines in (0, 2):
                cases.append((_block_of(rng, first + 128 * lines + tail), a))
    for first in sizes[:6]:                          # no interior line, no tail
        cases.append((_block_of(rng, first), 128 - first))
    for want, a in ((5, 3), (100, 20), (127, 1), (2, 127), (100, 100), (64, 65), (17, 120)):
        cases.append((_block_of(rng, want), a))
    assert len(cases) == 98 + 6 + 7
    _run(gpu, cases)


def test_last_flush_crosses_a_line(gpu, force):
    # The last two ops are 64-byte pieces taken in one trip: the last whole
    # line and the tail go out as two jobs, a trip apart.
    force("decoder", "ring")
    rng = random.Random(307)
    cases = []
    for k in range(64):
        body = 300 + 13 * k
        s = _prefix(Stream(rng), body, 20)
        s.copy(64, 64 + k).lit(60) if k % 2 else s.lit(60).copy(64, 200)
        # dst + made sits 1 + k % 100 bytes below a line before the two ops
        a = (-(body + 1 + k % 100)) % 128
        cases.append((s.done(), a))
    _run(gpu, cases)


def test_all_lanes_refill(gpu, force):
    # 64 blocks of one long literal: every lane asks for a refill in the same
    # trips (32 jobs a trip are served); streams that end 1, 15, 16 and 17
    # bytes into a 64-byte refill chunk, and on its boundary.
    force("decoder", "ring")
    rng = random.Random(308)
    cases = []
    for k in range(64):
        r = (1, 15, 16, 17, 0)[k % 5]
        slen = 64 * (10 + k % 7) + r
        s = Stream(rng).lit(slen - 5)                # header 2, tag 3
        out = s.done()
        assert len(out) == slen
        cases.append((out, _spread(k)))
    _run(gpu, cases)
    # ... and beside blocks of short ops, in two workgroups
    mixed = []
    for k, c in enumerate(cases):
        mixed += [c, (_at(rng, 3 * k, "copy", 1 + k, 64 + k), _spread(k + 1))]
    _run(gpu, mixed)
