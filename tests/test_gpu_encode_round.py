"""The encoder's round (lgs_encode.hip, encode_pass), step by step.

Blocks built so that each step of the round meets its edge -- the match test
(which lane may match), the match extension (where a copy ends), the op
record (the 64-op flush) and batches without a match -- each through the
host batch, the device batch (1, 2, 65 and 130 blocks a launch) and the
drop-in, byte for byte against the reference encoder, and round-tripped
through the reference decoder.

The second pass of encode_chunk (every batch swapping lane by lane) is never
taken on gfx950 by itself: the probe library has a switch for it
(lgs_probe_encode_second_pass), and test_second_pass_in_probe_child runs the
probe cases of this file in a child process that loads that library
(conftest.py, LGS_TEST_PROBE=1), as tests/test_gpu_probe_decoders.py does for
the probe decoders.
"""
from __future__ import annotations

import os
import random
import re
import subprocess
import sys

import pytest

import oracle
from encode_helpers import _copies, _device_batch, _other, _probe_offsets, _rnd
from lcdb_amd import corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.environ.get("LGS_TEST_PROBE") == "1"

SIZES = [17, 18, 255, 256, 257, 2047, 2048, 2049, 4096, 4208, 16384, 65536, 65536 + 17,
         65536 + 16, 131072 + 100]


def _mixed(rng: random.Random, n: int) -> bytes:
    """n bytes of tokens from a small vocabulary: copies of many lengths and
    distances, literals in between."""
    vocab = [_rnd(rng, rng.randrange(3, 13)) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(vocab) if rng.randrange(4) else _rnd(rng, rng.randrange(1, 9))
    return bytes(out[:n])


def _after_copy(rng: random.Random):
    """A 24-byte head: 16 random bytes P (positions 1..15 probed and entered),
    then P[4:12] again -- a copy found at 16 that ends at 24."""
    p = _rnd(rng, 16)
    return p, p + p[4:12]


def _exact_copy(rng: random.Random, length: int, end: bool = False) -> bytes:
    """A far copy of exactly `length` bytes: M enters the table at its first
    byte (position 12, a probe of the first search), and comes again one byte
    after a copy's end, where the next search's first probe stands.  That
    copy is a run of one byte, long enough for two probes of the search that
    has crossed M to fall into it."""
    q = _rnd(rng, 1)
    k = _rnd(rng, 12, avoid=q)
    m = _rnd(rng, length, avoid=q)
    x = _other(rng, q[0])
    y = _other(rng, x[0], q[0])
    z = _other(rng, q[0], m[0])
    run = q * (3 * ((length + 60) >> 5) + 12)
    return k + m + x + run + z + m + (b"" if end else y + _rnd(rng, 20, avoid=q))


def _run(rng: random.Random, period: int, length: int, end: bool = False) -> bytes:
    """A copy of exactly `length` bytes at distance `period`: a run of
    period + length bytes found at its second period."""
    unit = _rnd(rng, period)
    run = (unit * (length // period + 2))[:period + length]
    brk = _other(rng, run[length % period])
    return _rnd(rng, 8, avoid=unit) + run + (b"" if end else brk + _rnd(rng, 20, avoid=unit))


def _records(rng: random.Random, copies: int) -> bytes:
    """`copies` 8-byte records, 4 new bytes and a 4-byte repeat each: one
    copy of 4 bytes per record.  (A record's last new byte is no other
    record's, or the repeat would be found a byte early, as 5 bytes.)"""
    g = _rnd(rng, 4)
    out = bytearray(_rnd(rng, 5, avoid=g) + g)
    lasts = rng.sample([b for b in range(1, 256) if b not in g], copies)
    prev = 0
    for k in range(copies):
        u = _other(rng, prev, *g) + _rnd(rng, 2, avoid=g) + bytes([lasts[k]])
        prev = u[0]
        out += u + g
    return bytes(out) + _rnd(rng, 16, avoid=g)           # (no match in the last 15 bytes)


def _pieces(copies: list[int], length: int) -> bool:
    """The stream's last copy, as emitted (64- and 60-byte pieces first,
    snappy.c:75-102), is one of `length` bytes."""
    return any(sum(copies[i:]) == length for i in range(len(copies)))


def _cases() -> list[tuple[str, bytes]]:
    rng = random.Random(0x5AA9)
    ref = oracle.best()
    offs = _probe_offsets(200)
    cases: list[tuple[str, bytes]] = []

    def add(name: str, b: bytes) -> None:
        cases.append((name, bytes(b)))

    def add_when(name: str, make, ok) -> None:
        # The table has as few as 256 entries, so a position entered for a
        # later match may be overwritten before it: draw until the reference's
        # stream has the copies the case is about.
        for _ in range(4000):
            b = make()
            if ok(_copies(ref.encode(b))):
                return add(name, b)
        raise AssertionError(name)

    # ---- sizes (table size steps, chunk restarts, the short tail chunk)
    for n in SIZES:
        add(f"size{n}", _mixed(rng, n))
    # ---- (b) the match test
    p, head = _after_copy(rng)
    # the search's first probe (lane 2) after a copy
    add("first_probe", head + _other(rng, p[12], p[0]) + p[1:9] + _rnd(rng, 20))
    # probe k of a search and no probe before it: after a copy, and in a
    # chunk's first search (k = 61 is lane 63; 62 and 124 start the second and
    # third batches, placed from the probe table)
    for k in (0, 1, 31, 32, 33, 47, 48, 49, 59, 60, 61, 62, 63, 123, 124, 125, 186):
        step = offs[k + 1] - offs[k]     # (a probe is made if the next one is inside the limit)

        def after_copy(k=k, step=step):
            p, head = _after_copy(rng)
            fill = _other(rng, p[12]) + _rnd(rng, offs[k], avoid=p)
            return head + fill + p[1:9] + _rnd(rng, 20 + step)
        add_when(f"after_copy_probe{k}", after_copy, lambda c: c == [8, 8])
        if offs[k] >= 8:                 # (the repeat is of position 1, the first entered)
            def first_search(k=k, step=step):
                x = _rnd(rng, 1 + offs[k])
                return x + x[1:9] + _rnd(rng, 20 + step)
            add_when(f"first_search_probe{k}", first_search, lambda c: c == [8])
    # lane B's 64-bit re-match (snappy.c:182): bytes at..at+3 entered before,
    # at+4..at+6 zero -- and the same with one of them not zero
    def b_case(z):
        p, head = _after_copy(rng)
        while p[1] == p[12]:
            p, head = _after_copy(rng)
        return head + p[1:5] + z + _rnd(rng, 24)
    add_when("b_rematch", lambda: b_case(b"\0\0\0"), lambda c: c == [8, 4])
    add_when("b_no_rematch0", lambda: b_case(b"\1\0\0"), lambda c: c == [8])
    add_when("b_no_rematch2", lambda: b_case(b"\0\0\1"), lambda c: c == [8])
    # A and B share a hash: a copy that ends inside a run of one byte
    for name, z in (("ab_share_rematch", b"\0\0\0"), ("ab_share", b"")):
        a = _rnd(rng, 1)
        pre = _rnd(rng, 10, avoid=a)
        add(name, pre + a * 4 + _rnd(rng, 7, avoid=a) + a * 9 + z + _rnd(rng, 24, avoid=a))
    # the only 4-byte match stands where lane A does (at - 1)
    def only_a():
        p, _ = _after_copy(rng)
        while p[3] == p[12]:
            p, _ = _after_copy(rng)
        p = p[:2] + p[11:12] + p[3:]
        return p + p[4:12] + p[3:6] + _other(rng, p[6]) + _rnd(rng, 24, avoid=p)
    add_when("only_a", only_a, lambda c: c == [8])
    # a repeat that starts 1..20 bytes before the block's end (probes past the
    # limit n - 15 must not match): in the first search and after a copy
    for t in range(1, 21):
        r = _rnd(rng, 48)
        add(f"tail_first{t}", r + r[1:1 + t])
        p, head = _after_copy(rng)
        add(f"tail_after_copy{t}", head + _other(rng, p[12]) + _rnd(rng, 24, avoid=p) + p[1:1 + t])
    # ---- (c) the extension
    for length in (4, 63, 64, 65, 67, 68, 127, 128, 129, 4000):
        ok = lambda c, length=length: _pieces(c, length)
        add_when(f"far_copy{length}", lambda: _exact_copy(rng, length), ok)
        add_when(f"period1_copy{length}", lambda: _run(rng, 1, length), ok)
        add_when(f"period3_copy{length}", lambda: _run(rng, 3, length), ok)
    for length in (20, 64, 70):
        ok = lambda c, length=length: _pieces(c, length)
        add_when(f"far_copy_to_end{length}", lambda: _exact_copy(rng, length, end=True), ok)
        add_when(f"period3_to_end{length}", lambda: _run(rng, 3, length, end=True), ok)
    add("run_to_chunk_end", _rnd(rng, 1000, avoid=b"xyz") + (b"xyz" * 22000)[:65536 - 1000])
    add("run_over_chunk_end", _rnd(rng, 1000, avoid=b"xyz") + (b"xyz" * 22000)[:65536 - 500]
        + _rnd(rng, 40))
    # ---- (d) the op record and its flush every 64 ops
    for k in (63, 64, 65, 128, 129):
        add_when(f"copies{k}", lambda: _records(rng, k), lambda c, k=k: c == [4] * k)
    # ---- batches without a match
    add("random4096", bytes(rng.randrange(256) for _ in range(4096)))
    add("random16384", bytes(rng.randrange(256) for _ in range(16384)))
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def expected():
    """The reference's bytes for every case, computed once."""
    ref = oracle.best()
    exp = {name: ref.encode(b) for name, b in CASES}
    for name, b in CASES:
        assert ref.decode(exp[name]) == b, name
    return exp


def test_cases_are_what_they_say(expected):
    # The inputs' own properties, read from the reference's streams.
    for length in (4, 63, 64, 65, 67, 68, 127, 128, 129, 4000):
        for kind in ("far", "period1", "period3"):
            assert _pieces(_copies(expected[f"{kind}_copy{length}"]), length), (kind, length)
    for k in (63, 64, 65, 128, 129):
        assert _copies(expected[f"copies{k}"]) == [4] * k, k
    assert _copies(expected["random4096"]) == [] and _copies(expected["random16384"]) == []
    assert _copies(expected["only_a"]) == [8]
    assert _copies(expected["b_rematch"]) == [8, 4]
    assert _copies(expected["b_no_rematch0"]) == [8] and _copies(expected["b_no_rematch2"]) == [8]
    for k in (31, 61, 62, 124, 186):
        assert _copies(expected[f"first_search_probe{k}"]) == [8], k
        assert _copies(expected[f"after_copy_probe{k}"]) == [8, 8], k


def _check(outs, names, expected, route):
    ref = oracle.best()
    for name, o in zip(names, outs):
        assert o == expected[name], (route, name)
    for name, o in zip(names[:8], outs[:8]):
        assert ref.decode(o) is not None, (route, name)


def _launches():
    """(label, case indices) of the device launches: every case is in one of
    each size class's launches; 1, 2, 65 and 130 blocks a launch."""
    small = [i for i, (_, b) in enumerate(CASES) if len(b) <= 4608]
    mid = [i for i, (_, b) in enumerate(CASES) if 4608 < len(b) <= 16896]
    big = [i for i, (_, b) in enumerate(CASES) if len(b) > 16896]
    out = [("small1", small[:1]), ("small2", small[1:3]), ("small65", small[3:68]),
           ("small130", (small[68:] + small)[:130]),
           ("mid1", mid[:1]), ("mid2", mid[1:3]), ("mid65", (mid + small)[:65]),
           ("big1", big[:1]), ("big2", big[1:3]),
           ("big65", (big[3:] + small[::3])[:65]), ("big130", (big[:2] + mid + small)[:130])]
    seen = {i for _, idx in out for i in idx}
    assert seen == set(range(len(CASES))), sorted(set(range(len(CASES))) - seen)
    return out


def test_round_host_batch(gpu, expected):
    names = [n for n, _ in CASES]
    _check(gpu.encode_batch_host([b for _, b in CASES]), names, expected, "host")


@pytest.mark.parametrize("label", [lb for lb, _ in _launches()])
def test_round_device_batch(gpu, expected, label):
    idx = dict(_launches())[label]
    names = [CASES[i][0] for i in idx]
    _check(_device_batch([CASES[i][1] for i in idx]), names, expected, label)


def test_round_dropin(gpu, expected):
    ref = oracle.best()
    for name, b in CASES:
        o = gpu.encode(b)
        assert o == expected[name], name
        assert ref.decode(o) == b, name


# ---- the second pass (probe library only) -----------------------------------

SECOND_PASS_CASES = [f"size{n}" for n in SIZES] + ["copies65"]

if PROBE:
    @pytest.mark.probe
    def test_second_pass_probe_library(gpu, expected):
        from lcdb_amd import _native
        lib = _native.lib()
        ref = oracle.best()
        byname = dict(CASES)
        blocks = [byname[n] for n in SECOND_PASS_CASES]
        c1 = corpus.fillseq(256)
        c1_ref = [ref.encode(b) for b in c1.blocks()]
        got = {}
        try:
            for on in (1, 0):
                _native.check(lib.lgs_probe_encode_second_pass(on), "lgs_probe_encode_second_pass")
                outs = gpu.encode_batch_host(blocks)                 # its own kernel classes
                for n, o in zip(SECOND_PASS_CASES, outs):
                    assert o == expected[n], (on, "host", n)
                small = [b for b in blocks if len(b) <= 4608]
                for k in (1, len(small)):                            # the <= 4 608-byte class
                    assert _device_batch(small[:k]) == [ref.encode(b) for b in small[:k]], (on, k)
                mid = [b for b in blocks if len(b) <= 16896]              # the <= 16 896-byte class
                assert _device_batch(mid) == [ref.encode(b) for b in mid], (on, "mid")
                # one launch of everything: the 64 KiB window kernel
                assert _device_batch(blocks) == [expected[n] for n in SECOND_PASS_CASES], on
                got[on] = _device_batch(c1.blocks())
                assert got[on] == c1_ref, (on, "C1")
        finally:
            lib.lgs_probe_encode_second_pass(0)
        assert got[1] == got[0]


def test_second_pass_in_probe_child():
    env = dict(os.environ, LGS_TEST_PROBE="1")
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-v", "-p", "no:cacheprovider",
                        "-m", "gpu and probe", "--timeout", "300", "--timeout-method", "thread",
                        os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    passed = set(re.findall(r"test_gpu_encode_round\.py::(\S+) PASSED", r.stdout))
    assert passed == {"test_second_pass_probe_library"}, (sorted(passed), tail)
    assert not re.search(r"\d+ (skipped|failed|error)", r.stdout), tail
