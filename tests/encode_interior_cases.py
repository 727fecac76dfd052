"""Blocks for the encoder's batch after a copy (lgs_encode.hip, encode_pass,
post_batch) and a pure-Python restatement of the reference parse that says
what each block does (tests/test_gpu_encode_interior.py).

The batch after a copy that ended at `at` has every lane on while
at <= n - 125 (kInterior); each case is named after its event and, where the
bound matters, after d = at - (n - 125): at d <= 0 every lane is a probe, at
d > 0 the kernel takes the lanes past the limit off.

`parse` is snappy.c:104-195 again, reporting per batch after a copy what the
round's lanes meet there: A's and B's 4-byte compares, B's 64-bit compare
(snappy.c:182), the search's matching probe and the end of the copy that
follows.  The CPU test holds its copy list to the reference encoder's stream
for every case before any of its reports is relied on.
"""
from __future__ import annotations

import random

from encode_helpers import _other, _probe_offsets, _rnd

K_HASH = 0x1E35A7BD
INTERIOR = 125                     # kMargin + 1 + probe_off(62)
OFFS = _probe_offsets(200)
INSIDE = -300                      # "well inside": at least 300 bytes more than the bound needs
DS = (-3, -2, -1, 0, 1, 2, 3, INSIDE)


def _ld32(b: bytes, i: int) -> int:
    return int.from_bytes(b[i:i + 4], "little")


def parse(x: bytes):
    """(copies, batches) of encode_block on x (one chunk, 17 <= len <= 65536).
    copies: (base, length, distance) as the parse makes them.  batches: one
    dict per re-probe after a copy (snappy.c:172-186) and the search behind it:
    at; a4 / b4: A's / B's 4 bytes equal their candidate's; bwide: the 64-bit
    compare accepts B; ab_share: A and B hash alike; probe: "B" for a re-match,
    the index of the search's matching probe, or None if the search ran out;
    copy_end: where the copy that follows ends (None without one)."""
    n = len(x)
    copies, batches = [], []
    assert 17 <= n <= 65536
    limit = n - 15
    size, shift = 256, 24
    while size < 2048 and size < n:
        size *= 2
        shift -= 1
    h = lambda v: ((v * K_HASH) & 0xFFFFFFFF) >> shift    # noqa: E731
    table = [0] * size
    pos = 1
    nxt = h(_ld32(x, pos))
    cur = None
    while True:
        skip, npos, k = 32, pos, 0
        while True:
            pos = npos
            npos = pos + (skip >> 5)
            skip += skip >> 5
            if npos > limit:
                return copies, batches
            cand = table[nxt]
            table[nxt] = pos
            nxt = h(_ld32(x, npos))
            if _ld32(x, pos) == _ld32(x, cand):
                break
            k += 1
        if cur is not None:
            cur["probe"] = k
        while True:
            base = pos
            pos += 4
            chk = cand + 4
            while pos < n and x[chk] == x[pos]:
                chk += 1
                pos += 1
            copies.append((base, pos - base, base - cand))
            if cur is not None and cur["copy_end"] is None:
                cur["copy_end"] = pos
            if pos >= limit:
                return copies, batches
            v = int.from_bytes(x[pos - 1:pos + 7], "little")
            lo = v & 0xFFFFFFFF
            ha = h(lo)
            a4 = _ld32(x, table[ha]) == lo
            table[ha] = pos - 1
            hb = h((v >> 8) & 0xFFFFFFFF)
            cand = table[hb]
            table[hb] = pos
            cur = {"at": pos, "a4": a4, "b4": _ld32(x, cand) == ((v >> 8) & 0xFFFFFFFF),
                   "bwide": (v >> 8) == _ld32(x, cand), "ab_share": ha == hb,
                   "probe": None, "copy_end": None}
            batches.append(cur)
            if not cur["bwide"]:
                nxt = h((v >> 16) & 0xFFFFFFFF)
                pos += 1
                break
            cur["probe"] = "B"


def pieces(copies) -> list[tuple[int, int, int]]:
    """The copies as emitted (snappy.c:75-102: 64-byte pieces while 68 or more
    are left, then 60 if more than 64 are), as (position, length, distance)."""
    out = []
    for base, ln, dist in copies:
        while ln >= 68:
            out.append((base, 64, dist))
            base, ln = base + 64, ln - 64
        if ln > 64:
            out.append((base, 60, dist))
            base, ln = base + 60, ln - 60
        out.append((base, ln, dist))
    return out


def _batch_at(b: bytes, at: int):
    for r in parse(b)[1]:
        if r["at"] == at:
            return r
    return None


def _mixed(rng: random.Random, n: int) -> bytes:
    """n bytes of tokens from a small vocabulary: copies of many lengths and
    distances, literals in between."""
    vocab = [_rnd(rng, rng.randrange(3, 13)) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(vocab) if rng.randrange(4) else _rnd(rng, rng.randrange(1, 9))
    return bytes(out[:n])


def _records(rng: random.Random, copies: int, avoid: bytes = b"") -> bytes:
    """`copies` 8-byte records, 4 new bytes and a 4-byte repeat each: one copy
    of 4 bytes per record, the last one ending the string."""
    if copies == 0:
        return b""
    g = _rnd(rng, 4, avoid=avoid)
    out = bytearray(_rnd(rng, 5, avoid=g + avoid) + g)
    lasts = rng.sample([b for b in range(1, 256) if b not in g + avoid], copies)
    prev = 0
    for k in range(copies):
        u = _other(rng, prev, *g, *avoid) + _rnd(rng, 2, avoid=g + avoid) + bytes([lasts[k]])
        prev = u[0]
        out += u + g
    return bytes(out)


class Case:
    """One block, the position of the batch it is about (None: no single
    batch) and what `parse` must report there: `want` maps a report's key to
    its value; `check` is a further condition on (copies, batches, block)."""

    def __init__(self, name, block, at=None, want=None, check=None):
        self.name, self.block, self.at = name, bytes(block), at
        self.want, self.check = want or {}, check

    def holds(self) -> bool:
        copies, batches = parse(self.block)
        if self.at is not None:
            r = next((r for r in batches if r["at"] == self.at), None)
            if r is None or any(r[k] != v for k, v in self.want.items()):
                return False
        return self.check is None or bool(self.check(copies, batches, self.block))

    @property
    def d(self):
        return None if self.at is None else self.at - (len(self.block) - INTERIOR)


def _draw(name: str, make) -> Case:
    """The first of `make`'s draws that holds what it says; none within the
    limit is an error (the table has as few as 256 entries, so a position
    entered for a later match may be overwritten before it)."""
    for _ in range(400):
        c = make()
        if c.holds():
            return c
    raise AssertionError(f"no block for {name}")


def _dname(d: int) -> str:
    return "inside" if d == INSIDE else f"d{d:+d}"


def cases() -> list[Case]:
    rng = random.Random(0x1A7E5)
    out: list[Case] = []
    pres = (0, 30, 140)            # records before the event: tables of 256, 512 and 2 048 entries

    def head(s: bytes, q: bytes, pre: bytes) -> tuple[bytes, int]:
        """pre + one byte + s + a run of q: s is probed byte by byte (the
        search after pre's last copy, or the chunk's first), the run is found
        at its second byte and copied to its end.  Returns the bytes and `at`,
        the position of whatever follows the run."""
        b = pre + _rnd(rng, 1, avoid=q + s) + s + q * 8
        return b, len(b)

    def fill(n: int, *avoid: bytes) -> bytes:
        return _rnd(rng, n, avoid=b"".join(avoid))

    def sized(b: bytes, at: int, d: int, *avoid: bytes) -> bytes:
        """b cut or filled so that at - (len - 125) = d."""
        n = at + INTERIOR - d
        assert len(b) <= n, (len(b), n)
        return b + fill(n - len(b), *avoid)

    def pre_of(i: int, *avoid: bytes) -> bytes:
        return _records(rng, pres[i % len(pres)], avoid=b"".join(avoid))

    # ---- lane B, each event on both sides of the bound and well inside
    def lane_b(name, after, want, i, d, s0_is_q=False, late_ok=None):
        def make():
            q = _rnd(rng, 1)
            s = _rnd(rng, 24, avoid=q)
            if s0_is_q:
                s = q + s[1:]
            b, at = head(s, q, pre_of(i, q, s))
            # B's four bytes are s[1:5], entered at s's second byte
            body = s[1:2] + after(s, q)
            w = dict(want)
            if late_ok is not None and not late_ok(d):
                w["probe"] = None            # the lane is past the limit: it must not match
            return Case(f"{name}_{_dname(d)}", sized(b + body, at, d, q, s), at, w)
        out.append(_draw(f"{name}_{_dname(d)}", make))

    def probe_ok(k):
        return lambda d: OFFS[k + 1] <= 109 - d       # snappy.c:143 for the search's probe k

    for i, d in enumerate(DS):
        # B's true re-match: at+4..at+6 zero, at+7 not
        lane_b("b_rematch", lambda s, q: s[2:5] + b"\0\0\0" + fill(1, q, s),
               {"b4": True, "bwide": True, "probe": "B"}, i, d)
        # B matches on four bytes, exactly one of at+4, at+5, at+6 is not zero
        for z in range(3):
            lane_b(f"b4_nz{z}", lambda s, q, z=z: s[2:5] + bytes(1 if j == z else 0 for j in range(3)),
                   {"b4": True, "bwide": False}, i + z, d)
        # B rejected, the search matches in the same batch
        lane_b("b_rej_search0", lambda s, q: s[2:10] + _other(rng, s[10]),
               {"b4": True, "bwide": False, "probe": 0}, i, d)

        def search1(s, q):       # s[1:5] = abcd and s[7:11] = cdef: at+2 repeats s[7:11], at+1 nothing
            return s[2:5] + s[9:11] + _other(rng, s[11])
        out.append(_draw(f"b_rej_search1_{_dname(d)}", lambda: _search1_case(rng, search1, pre_of, i, d, head, sized)))
        for k in (30, 61):
            lane_b(f"b_rej_search{k}",
                   lambda s, q, k=k: s[2:5] + b"\1" + fill(OFFS[k] - 4, q, s) + s[8:16] + _other(rng, s[16]),
                   {"b4": True, "bwide": False, "probe": k}, i + k, d, late_ok=probe_ok(k))
        # A and B share a hash: the copy ends inside a run of one byte
        for nm, z, w in (("ab_share_rematch", b"\0\0\0", {"bwide": True, "probe": "B"}),
                         ("ab_share_rej", b"\1\0\0", {"bwide": False})):
            def make(nm=nm, z=z, w=w, i=i, d=d):
                a = _rnd(rng, 1)
                pre = pre_of(i, a)
                b = pre + fill(10, a) + a * 4 + fill(7, a) + a * 8
                at = len(b) - 4
                return Case(f"{nm}_{_dname(d)}", sized(b + z + fill(1, a), at, d, a), at,
                            dict(w, b4=True, ab_share=True))
            out.append(_draw(f"{nm}_{_dname(d)}", make))
        # the only 4-byte match stands at lane A
        lane_b("only_a", lambda s, q: s[2:4] + _other(rng, s[4]),
               {"a4": True, "b4": False, "probe": None}, i, d, s0_is_q=True)
        # B rejected and nothing in the batch matches; near the bound the search then runs out
        lane_b("b_rej_nomatch", lambda s, q: s[2:5] + b"\1",
               {"b4": True, "bwide": False, "probe": None}, i, d)
    # B rejected, no lane matches, the match comes from the second or third
    # batch: probe k is made while OFFS[k + 1] <= 109 - d, so these stand as
    # near the bound as they can, one byte further in, and well inside.
    for k in (62, 63, 124):
        dmax = 109 - OFFS[k + 1]
        for i, d in enumerate((dmax, dmax - 1, min(INSIDE, dmax - 300))):
            nm = f"b_rej_late{k}_" + ("inside" if i == 2 else f"d{d:+d}")

            def make(k=k, d=d, nm=nm, i=i):
                q = _rnd(rng, 1)
                s = _rnd(rng, 24, avoid=q)
                b, at = head(s, q, pre_of(i, q, s))
                body = s[1:5] + b"\1" + fill(OFFS[k] - 4, q, s) + s[8:16] + _other(rng, s[16])
                return Case(nm, sized(b + body, at, d, q, s), at, {"b4": True, "bwide": False, "probe": k})
            out.append(_draw(nm, make))

    # ---- the extension's end: a far copy found by an all-lanes batch
    def far(name, length, kk, tail_len, i, to_end=False):
        """12 bytes, M, three zeros (what the image holds past the chunk: only
        the end mask stops a copy of M that ends the chunk), a run, then M
        again at the search's probe kk and `tail_len` bytes."""
        def make():
            q = _rnd(rng, 1)
            m = _rnd(rng, length, avoid=q)
            pre = pre_of(i, q)
            b = pre + fill(12, q) + m + b"\0\0\0" + _other(rng, q[0]) + q * (3 * ((length + 60) >> 5) + 12)
            at = len(b)
            b += _other(rng, q[0], m[0]) + fill(OFFS[kk], q, m[:4])
            base = len(b)
            b += m + (b"" if to_end else fill(tail_len, q))
            n = len(b)

            def check(copies, batches, blk, base=base, at=at, n=n):
                return (copies[-1][0] == base and copies[-1][1] == length and at <= n - INTERIOR
                        and copies[-1][0] + copies[-1][1] == n - (0 if to_end else tail_len))
            return Case(name, b, at, {"probe": kk, "copy_end": base + length}, check)
        out.append(_draw(name, make))

    for t in range(21):
        far(f"ext_end_t{t}", 130, 0, t, t, to_end=(t == 0))
    for i, length in enumerate((4, 60, 61, 64, 65, 67, 68, 124, 128, 129)):
        far(f"ext_len{length}", length, 0, 300, i)
    # the first step's window against the chunk's end: n - (base + 4) = E
    for i, (e, kk) in enumerate(((63, 45), (64, 44), (65, 44), (127, 0), (128, 0), (129, 0))):
        far(f"ext_edge{e}", e + 4, kk, 0, i, to_end=True)

    # ---- the restore store: the match at lane m, a later lane's entry needed again
    for i, lane in enumerate((2, 3, 31, 32, 33, 62, 63)):
        k = lane - 2
        j = OFFS[k + 1] - OFFS[k]        # the first later lane stands j bytes into the copy

        def make(k=k, j=j, lane=lane, i=i):
            q = _rnd(rng, 1)
            s = _rnd(rng, 24, avoid=q)
            pre = pre_of(i, q, s)
            b, at = head(s, q, pre)
            src = len(pre) + 1                       # where s stands
            b += _other(rng, q[0], s[0]) + fill(OFFS[k], q, s)
            base = len(b)
            b += s[:20] + _other(rng, s[20], q[0]) + fill(3, q, s)
            v = len(b)
            b += s[j:j + 6] + _other(rng, s[j + 6], q[0]) + fill(300, q, s)

            def check(copies, batches, blk, base=base, v=v, w=src + j):
                return (base, 20, base - src) in copies and (v, 6, v - w) in copies
            return Case(f"restore_lane{lane}", b, at, {"probe": k, "copy_end": base + 20}, check)
        out.append(_draw(f"restore_lane{lane}", make))
    # token soup over the table-size steps and both LDS image classes
    for n in (124, 125, 126, 127, 140, 141, 142, 200, 255, 256, 257, 2047, 2048, 2049, 4096, 4208,
              4608, 4609, 16896):
        out.append(Case(f"soup{n}", _mixed(rng, n)))

    # ---- the record: the 64-op flush in the interior
    for k in (63, 64, 65, 129):
        def make(k=k):
            b = _records(rng, k)
            b += fill(300, b[5:9])
            n = len(b)

            def check(copies, batches, blk, k=k, n=n):
                return [c[1] for c in copies] == [4] * k and batches[min(k, 64) - 1]["at"] <= n - INTERIOR
            return Case(f"copies{k}", b, None, None, check)
        out.append(_draw(f"copies{k}", make))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def _search1_case(rng, after, pre_of, i, d, head, sized) -> Case:
    """B rejected and the search's probe 1 matches: s[1:5] = abcd, s[7:11] =
    cdef, and the block goes on a, bcd, ef after the run -- B finds abcd with e
    behind it, probe 0 finds nothing (bcde), probe 1 finds cdef."""
    q = _rnd(rng, 1)
    s = bytearray(_rnd(rng, 24, avoid=q))
    s[7:9] = s[3:5]
    s = bytes(s)
    b, at = head(s, q, pre_of(i, q, s))
    body = s[1:2] + after(s, q)
    return Case(f"b_rej_search1_{_dname(d)}", sized(b + body, at, d, q, s), at,
                {"b4": True, "bwide": False, "probe": 1})
