"""The pair decoder (decode_pair_kernel: a walking and a moving wave per 64
blocks) on streams built op by op, forced through the "ring"
route so that small batches reach it.  Every case compares status and bytes
with the reference's decode."""
from __future__ import annotations

import random

import numpy as np
import pytest

import oracle
from decode_helpers import Stream, _header, _varint  # noqa: F401

pytestmark = pytest.mark.gpu

CAP = 4608
COUNTS = (1, 2, 63, 64, 65, 128, 129, 193)


ONE_TAG = _varint(5) + bytes([4 << 2]) + b"hello"


def _tiny_ops(rng, n_ops: int) -> bytes:
    # n_ops one-byte ops: a literal byte, then copies of it and fresh bytes
    s = Stream(rng).lit(1)
    for k in range(n_ops - 1):
        if k % 3 == 2:
            s.lit(1)
        else:
            s.copy(1, 1 + (k % 2 if len(s.out) > 1 else 0))
    return s.done()


def _short_tag_run(rng, n_tags: int) -> bytes:
    # >= 600 two- and three-byte tags: the op queue fills
    s = Stream(rng).lit(16)
    for k in range(n_tags):
        if k % 2:
            s.copy(4 + k % 3, 1 + k % 16, form=1)
        else:
            s.copy(1 + k % 7, 1 + k % 13, form=2)
    return s.done()


def _literal_run(rng, sizes) -> bytes:
    s = Stream(rng)
    for n in sizes:
        s.lit(n)
    return s.done()


def _wrap_tag(rng, at: int, ring: int) -> bytes:
    # A five-byte tag (COPY4) that starts at stream offset `at` (mod ring):
    # its bytes straddle the input ring's wrap for at = ring - 4 .. ring - 1
    # (the pair kernel's ring is 192 bytes, decode_ring_kernel's 128).
    s = Stream(rng).lit(40)
    for _ in range(3):                      # three laps of the ring
        gap = (at - (s.pos() + 2)) % ring   # (+2: the varint header of >= 128 bytes)
        if gap < 2:
            gap += ring
        while gap:                          # literals of n bytes: n + 1 stream bytes
            step = min(gap, 61)
            if gap - step == 1:
                step -= 1
            s.lit(step - 1)
            gap -= step
        assert (s.pos() + 2) % ring == at
        s.copy(33, 37, form=3)
        s.copy(9, 9, form=3)
    out = s.done()
    assert len(_varint(len(s.out))) == 2
    return out


def _pad_to_64(rng, s: Stream) -> bytes:
    # stream length (header included) an exact multiple of 64
    assert len(s.out) >= 128                # (a two-byte header from here on)
    while True:
        r = (-(2 + len(s.body))) % 64
        if r == 0:
            out = s.done()
            assert len(out) % 64 == 0
            return out
        s.lit(r - 1 if 2 <= r <= 61 else 1 if r == 1 else 30)


def _far_copies(rng, dist: int, lens) -> bytes:
    s = Stream(rng).lit(dist)
    for n in lens:
        s.copy(n, dist if dist <= len(s.out) else len(s.out), form=2)
        s.lit(3)
    return s.done()


def _far_runs(rng, dist: int) -> bytes:
    # Several 64-byte far copies in a row, no op between them: each is taken
    # in the mover's first slot right after the flush and the landing of the
    # one before it, and waits across the barrier with the second slot idle.
    s = Stream(rng).lit(dist)
    for run in ((4, 5) if dist > 2000 else (4, 5, 9, 12)):
        for _ in range(run):
            s.copy(64, dist, form=2)
        s.lit(3)
    assert len(s.out) <= CAP
    return s.done()


def _far_after_burst(rng) -> bytes:
    # Output bursts (64-byte pieces, two a trip) and then far copies whose
    # source is what was just produced: not yet flushed when they are parsed.
    s = Stream(rng).lit(300)
    for d in (241, 250, 256, 257, 300):
        s.lit(64).lit(64).copy(64, 1).copy(64, d).copy(17, d).lit(60).copy(48, d + 7)
    return s.done()


def _near_overlaps(rng) -> list[bytes]:
    res = []
    for d in (1, 2, 3, 4, 5, 8, 15, 16, 17):
        s = Stream(rng).lit(max(d, 20))
        for n in (64, 63, 49, 48, 33, 32, 17, 16, 15, 5, 2, 1, 64, 64):
            s.copy(n, d)
            s.lit(1 + n % 5)
        res.append(s.done())
    return res


def _rejects(rng) -> list[bytes]:
    """Every reject of parse_tag at the first tag and at a tag deep in the
    stream (ops queued before it are in flight), truncations, and streams
    that do not end at want."""
    bad_tags = [
        bytes([2, 0, 0]),                                           # dist 0
        bytes([(9 << 2) | 2, 0xff, 0xff]),                          # dist > made
        bytes([(63 << 2) | 3]) + (2**31).to_bytes(4, "little"),     # dist >= 2^31
        bytes([63 << 2]) + b"\xff\xff\xff\x7f",                     # literal length 2^31
        bytes([62 << 2, 0xff, 0xff]),                               # header past the stream
        bytes([61 << 2, 0x10]),                                     # length bytes cut
        bytes([20 << 2]) + b"short",                                # literal past the stream
        bytes([1]),                                                 # COPY1 cut
        bytes([2, 1]),                                              # COPY2 cut
        bytes([3, 1, 0, 0]),                                        # COPY4 cut
    ]
    res = []
    for bad in bad_tags:
        res.append(_varint(100) + bad)
        deep = Stream(rng).lit(50)
        for k in range(120):
            deep.copy(1 + k % 64, 1 + k % 50).lit(1 + k % 9)
        res.append(_varint(len(deep.out) + 70) + bytes(deep.body) + bad)
    # a copy or a literal past want, deep
    s = Stream(rng).lit(200).copy(64, 100).copy(64, 150)
    res.append(s.done(want=len(s.out) - 1))
    res.append(s.done(want=len(s.out) + 1))                         # made != want at the end
    res.append(s.done(want=len(s.out) - 64))
    good = _short_tag_run(rng, 300)
    res += [good[:-1], good[:-2], good[:1], good[:2]]               # cut short
    lit = _literal_run(rng, [60, 61, 200, 3])
    res += [lit[:-1], lit[:-4]]
    res += [b"", b"\x00", b"\x80", b"\x80\x80\x80\x80\x80", _varint(CAP + 1) + b"\x00a",
            _varint(2**31) + b"\x00a", _varint(0) + b"\x00x"]
    return res


_POOL = None


def _pool():
    """The valid and the corrupt streams of every family, built once."""
    global _POOL
    if _POOL is None:
        rng = random.Random(20261)
        walk = [_short_tag_run(rng, 700), _literal_run(rng, [60, 61, 62, 63, 64] * 12),
                _literal_run(rng, [129, 192, 193, 4000]), _literal_run(rng, [64] * 64)]
        for ring in (192, 128):
            walk += [_wrap_tag(rng, (ring - 5 + k) % ring, ring) for k in range(6)]
        for k in range(4):
            s = Stream(rng).lit(70 + k)
            for j in range(40 + k):
                s.copy(1 + (7 * j + k) % 64, 1 + (11 * j) % 70).lit(1 + j % 61)
            walk.append(_pad_to_64(rng, s))
        far = [_far_after_burst(rng)]
        for d in (241, 256, 257, 4000):
            far.append(_far_copies(rng, d, (1, 16, 17, 48, 64)))
            far.append(_far_copies(rng, d, (64,) * 9))
        far += [_far_runs(rng, d) for d in (241, 256, 257, 4000)]
        far += _near_overlaps(rng)
        _POOL = ([ONE_TAG, b"\x00", _tiny_ops(rng, 3000)] + walk + far, _rejects(rng), walk, far)
    return _POOL


_REF = {}


def _expected(s: bytes):
    if s not in _REF:
        _REF[s] = oracle.best().decode(s) if s else None
    return _REF[s]


def _check(gpu, streams, cap: int = CAP) -> int:
    res, st = gpu.decode_batch_host(streams, [cap] * len(streams))
    oks = 0
    for k, (s, o, code) in enumerate(zip(streams, res, st)):
        exp = _expected(s)
        h = _header(s)
        if h is not None and h > cap:
            assert code == gpu.LGS_ST_NOSPACE, k
        elif exp is None:
            assert code == gpu.LGS_ST_CORRUPT, k
        else:
            assert code == gpu.LGS_ST_OK and o == exp, (k, len(s), len(exp))
            oks += 1
    return oks


def test_pool_is_what_it_says():
    # (no device needed for this one, but it guards the cases below)
    valid, bad = _pool()[:2]
    for s in valid:
        assert _expected(s) is not None and len(_expected(s)) <= CAP
    assert len(_pool()[0][2]) > 2 * 3000                       # thousands of one-byte ops
    assert any(len(s) % 64 == 0 for s in valid)
    n_bad = sum(_expected(s) is None for s in bad)
    assert n_bad >= len(bad) - 4                               # (the no-space ones decode)


@pytest.mark.parametrize("n", COUNTS)
def test_block_counts_every_family(gpu, force, n):
    # Lanes without a block, a second workgroup with one block, a whole
    # workgroup past `count`: n blocks drawn from every family in turn,
    # starting at a different family per count.
    force("decoder", "ring")
    valid, bad = _pool()[:2]
    allv = valid + bad
    streams = [allv[(n + k) % len(allv)] for k in range(n)]
    _check(gpu, streams)
    if n <= 2:
        for s in valid:                                       # every valid stream alone
            assert _check(gpu, [s] * n) == n


@pytest.mark.parametrize("lane,n", [(0, 64), (63, 64), (64, 65), (64, 128), (130, 193)])
def test_uneven_lives(gpu, force, lane, n):
    # One block of several thousand one-byte ops beside one-tag blocks, an
    # empty block and a zero-length input: the workgroup lives as long as
    # its longest block, the others' lanes idle without disturbing it.
    force("decoder", "ring")
    long_block = _pool()[0][2]
    streams = [ONE_TAG] * n
    streams[lane] = long_block
    streams[(lane + 1) % n] = b"\x00"
    streams[(lane + 7) % n] = b""
    assert _check(gpu, streams) == n - 1


def test_walker_ahead_and_behind(gpu, force):
    # The queue fills (runs of short tags), the walker waits for input (runs
    # of 60-64-byte literals, literals longer than the input ring), tags
    # across the ring's wrap, stream lengths that are multiples of 64: each
    # family beside every other in one workgroup, and each filling one.
    force("decoder", "ring")
    fam = _pool()[2]
    assert _check(gpu, (fam * 9)[:129]) == 129
    for s in fam:
        assert _check(gpu, [s] * 64 + [ONE_TAG]) == 65


def test_far_and_near_copies(gpu, force):
    # Distances 241, 256, 257 and 4 000 (beyond the ring: read back from the
    # flushed output) with lengths 1, 16, 17, 48, 64, 64-byte far copies
    # with a literal between them and in runs of 4 to 12 with none, far
    # copies of bytes produced in the same trip, and overlapping near copies
    # of every small period.
    force("decoder", "ring")
    fam = _pool()[3]
    assert len(fam) == 1 + 8 + 4 + 9
    assert _check(gpu, (fam * 8)[:130]) == 130
    for s in fam:
        assert _check(gpu, [s] * 65) == 65


def test_rejects_leave_neighbours_alone(gpu, force):
    # Every reject, first tag and deep, one per workgroup position in turn,
    # between valid blocks whose bytes must be untouched.
    force("decoder", "ring")
    valid, bad = _pool()[:2]
    streams = []
    for k, b in enumerate(bad):
        streams += [valid[(k + j) % len(valid)] for j in range(3)] + [b]
    assert len(streams) <= 300
    oks = _check(gpu, streams)
    assert oks >= 3 * len(bad)
    # a workgroup of rejects only, and rejects in every lane but one
    _check(gpu, (bad * 3)[:64])
    assert _check(gpu, (bad * 3)[:63] + [valid[3]]) >= 1


@pytest.mark.parametrize("shift", [1, 7, 13])
def test_alignment(gpu, force, shift):
    # Inputs and outputs `shift` bytes off 16-byte alignment (the output ring
    # is placed by the destination's alignment; refills and far copies read
    # at any byte address).
    import torch
    force("decoder", "ring")
    valid, bad = _pool()[:2]
    streams = (valid + bad[:12])[:70]
    lens = np.array([len(s) for s in streams], dtype=np.uint32)
    stride_in = (int(lens.max()) + 31) & ~15
    stride_out = CAP + 32
    n = len(streams)
    buf = np.zeros(n * stride_in + 64, dtype=np.uint8)
    in_off = np.arange(n, dtype=np.uint64) * np.uint64(stride_in) + np.uint64(shift)
    for s, o in zip(streams, in_off):
        buf[int(o):int(o) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    out_off = np.arange(n, dtype=np.uint64) * np.uint64(stride_out) + np.uint64(shift)
    dev = "cuda"
    d_in = torch.from_numpy(buf).to(dev)
    d_out = torch.full((n * stride_out + 64,), 0xEE, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    gpu.decode_batch(d_in, torch.from_numpy(in_off.view(np.int64)).to(dev),
                     torch.from_numpy(lens.view(np.int32)).to(dev), d_out,
                     torch.from_numpy(out_off.view(np.int64)).to(dev),
                     torch.full((n,), CAP, dtype=torch.int32, device=dev), d_len, d_st, CAP)
    torch.cuda.synchronize()
    out, olen, st = d_out.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy()
    for k, s in enumerate(streams):
        exp = _expected(s)
        o = int(out_off[k])
        if exp is None:
            assert st[k] == gpu.LGS_ST_CORRUPT, k
        elif len(exp) > CAP:
            assert st[k] == gpu.LGS_ST_NOSPACE, k
        else:
            assert st[k] == gpu.LGS_ST_OK and int(olen[k]) == len(exp), k
            assert out[o:o + len(exp)].tobytes() == exp, k
            # nothing written past the block's capacity or before its start
            assert (out[o + CAP:o + stride_out] == 0xEE).all(), k
            assert (out[o - shift:o] == 0xEE).all(), k
