"""Snappy streams built op by op for the decoder tests (tag forms:
snappy.c:53-110), and a plain walk over a stream's tags that the CPU tests
use to recompute what a case claims about its own bytes."""
from __future__ import annotations


def _varint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _header(s: bytes):
    v = 0
    for k in range(min(5, len(s))):
        v |= (s[k] & 0x7F) << (7 * k)
        if not s[k] & 0x80:
            return v if v <= 0x7FFFFFFF else None
    return None


def _lit_header(n: int, hdr: int | None = None) -> bytes:
    """The header of an n-byte literal in `hdr` bytes (the tag and 0-4 length
    bytes); None: the shortest form.  A longer form than needed is legal."""
    m = n - 1
    if hdr is None:
        hdr = 1 if m < 60 else 2 if m < 256 else 3 if m < 65536 else 4 if m < (1 << 24) else 5
    if hdr == 1:
        assert m < 60
        return bytes([m << 2])
    assert 2 <= hdr <= 5 and m < (1 << (8 * (hdr - 1)))
    return bytes([(58 + hdr) << 2]) + m.to_bytes(hdr - 1, "little")


def _lit(b: bytes) -> bytes:
    # literal tag, snappy.c:53-73 header forms (1-3 length bytes here)
    n = len(b) - 1
    if n < 60:
        return bytes([n << 2]) + b
    if n < 256:
        return bytes([60 << 2, n]) + b
    if n < 65536:
        return bytes([61 << 2, n & 255, n >> 8]) + b
    return bytes([62 << 2, n & 255, (n >> 8) & 255, n >> 16]) + b


def _copy2(length: int, dist: int) -> bytes:
    return bytes([((length - 1) << 2) | 2, dist & 255, dist >> 8])


class Stream:
    """A Snappy body grown op by op, with the output it decodes to.

    hlen: the length of the varint header that done() will write, for
    offset(); done() asserts it."""

    def __init__(self, rng, hlen: int | None = None):
        self.rng, self.body, self.out = rng, bytearray(), bytearray()
        self.hlen = hlen

    def lit(self, n: int, hdr: int | None = None, data: bytes | None = None) -> "Stream":
        """An n-byte literal; hdr: its header's size in bytes (1-5, the tag
        included), None for the shortest."""
        b = self.rng.randbytes(n) if data is None else data
        assert len(b) == n and n >= 1
        if hdr is None:
            m = n - 1
            if m < 60:
                self.body.append(m << 2)
            elif m < 256:
                self.body += bytes([60 << 2, m])
            elif m < 65536:
                self.body += bytes([61 << 2, m & 255, m >> 8])
            else:
                self.body += _lit_header(n)
        else:
            self.body += _lit_header(n, hdr)
        self.body += b
        self.out += b
        return self

    def copy(self, n: int, d: int, form: int = 2) -> "Stream":
        assert 1 <= n <= 64 and 1 <= d <= len(self.out)
        if form == 1:
            assert 4 <= n <= 11 and d < 2048
            self.body += bytes([((d >> 8) << 5) | ((n - 4) << 2) | 1, d & 255])
        elif form == 2:
            assert d < 65536
            self.body += bytes([((n - 1) << 2) | 2, d & 255, d >> 8])
        else:
            self.body += bytes([((n - 1) << 2) | 3]) + d.to_bytes(4, "little")
        if d >= n:
            self.out += self.out[len(self.out) - d:len(self.out) - d + n]
        else:
            for _ in range(n):
                self.out.append(self.out[-d])
        return self

    def raw(self, b: bytes) -> "Stream":
        """Bytes appended to the body as they are (a tag the builder would
        not write: its output is not modelled)."""
        self.body += b
        return self

    def pos(self) -> int:
        """Stream offset of the next tag (the header is 1 byte below 128
        output bytes and 2 bytes from there to 16 383)."""
        return len(self.body)

    def offset(self) -> int:
        """Stream offset of the next tag, the varint header included."""
        assert self.hlen is not None
        return self.hlen + len(self.body)

    def made(self) -> int:
        return len(self.out)

    def done(self, want: int | None = None) -> bytes:
        h = _varint(len(self.out) if want is None else want)
        assert self.hlen is None or want is not None or len(h) == self.hlen
        return h + bytes(self.body)


def hlen_for(want: int) -> int:
    return len(_varint(want))


def walk(s: bytes):
    """The tags of a stream, as the format defines them, up to the first one
    that does not fit: (want, ops, clean), ops a list of dicts with
      kind   0 literal, 1 / 2 / 4 the copy forms
      at     stream offset of the tag
      lm     stream offset just past a copy's tag or a literal's header
      end    stream offset of the next tag
      made   output length before the op
      n      bytes it makes
      dist   a copy's distance (0 for a literal)
    clean: the walk consumed the stream exactly and every op was in bounds."""
    want = _header(s)
    if want is None:
        return None, [], False
    p = 1
    while s[p - 1] & 0x80:
        p += 1
    ops, made = [], 0
    while p < len(s):
        tag = s[p]
        kind = tag & 3
        if kind == 0:
            m, hl = tag >> 2, 1
            if m >= 60:
                extra = m - 59
                if p + 1 + extra > len(s):
                    return want, ops, False
                m = int.from_bytes(s[p + 1:p + 1 + extra], "little")
                hl += extra
            n = m + 1
            op = dict(kind=0, at=p, lm=p + hl, end=p + hl + n, made=made, n=n, dist=0)
            if op["end"] > len(s):
                return want, ops, False
        else:
            chl = {1: 2, 2: 3, 3: 5}[kind]
            if p + chl > len(s):
                return want, ops, False
            if kind == 1:
                n, dist = 4 + ((tag >> 2) & 7), ((tag & 0xE0) << 3) | s[p + 1]
            else:
                n, dist = 1 + (tag >> 2), int.from_bytes(s[p + 1:p + chl], "little")
            op = dict(kind={1: 1, 2: 2, 3: 4}[kind], at=p, lm=p + chl, end=p + chl, made=made,
                      n=n, dist=dist)
            if dist == 0 or dist > made:
                return want, ops, False
        if made + op["n"] > want:
            return want, ops, False
        ops.append(op)
        made += op["n"]
        p = op["end"]
    return want, ops, made == want


def run_ahead(s: bytes):
    """S of the wave decoder's in-place bound: the largest
    made_before + slen - lm over the ops, and the ops that attain it."""
    _, ops, _ = walk(s)
    vals = [op["made"] + len(s) - op["lm"] for op in ops]
    best = max(vals)
    return best, [op for op, v in zip(ops, vals) if v == best]
