"""Helpers shared by the encoder's case files (test_gpu_encode_round.py,
test_gpu_encode_window.py): byte generators, the reference's probe
schedule, a parser of Snappy streams and the device-batch route."""
from __future__ import annotations

import random

import numpy as np

from lcdb_amd import corpus


def _probe_offsets(count: int) -> list[int]:
    """snappy.c:138-143: offset of the search's probe k from its first."""
    offs, at, skip = [], 0, 32
    for _ in range(count):
        offs.append(at)
        step = skip >> 5
        skip += step
        at += step
    return offs


def _rnd(rng: random.Random, n: int, avoid: bytes = b"") -> bytes:
    """n random bytes, none of them zero or in `avoid`."""
    alpha = [b for b in range(1, 256) if b not in avoid]
    return bytes(rng.choice(alpha) for _ in range(n))


def _other(rng: random.Random, *not_these: int) -> bytes:
    return bytes([rng.choice([b for b in range(1, 256) if b not in not_these])])


def _elements(stream: bytes) -> list[tuple[int, int, int]]:
    """The elements of a Snappy stream after its length header, as (output
    position, length, distance); a literal's distance is 0."""
    at, pos, out = 0, 0, []
    while stream[at] & 0x80:
        at += 1
    at += 1
    while at < len(stream):
        tag = stream[at]
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            at += 1
            if ln >= 60:
                nb = ln - 59
                ln = int.from_bytes(stream[at:at + nb], "little")
                at += nb
            ln += 1
            at += ln
            dist = 0
        elif kind == 1:
            ln = ((tag >> 2) & 7) + 4
            dist = ((tag >> 5) << 8) | stream[at + 1]
            at += 2
        else:
            nb = 2 if kind == 2 else 4
            ln = (tag >> 2) + 1
            dist = int.from_bytes(stream[at + 1:at + 1 + nb], "little")
            at += 1 + nb
        out.append((pos, ln, dist))
        pos += ln
    return out


def _copy_ops(stream: bytes) -> list[tuple[int, int, int]]:
    """(output position, length, distance) of the copy elements of a stream."""
    return [e for e in _elements(stream) if e[2]]


def _copies(stream: bytes) -> list[int]:
    """Lengths of the copy elements of a Snappy stream."""
    return [ln for _, ln, _ in _copy_ops(stream)]


def _device_batch(blocks: list[bytes]) -> list[bytes]:
    import torch
    from lcdb_amd import batch
    parts = []
    for b in blocks:
        a = np.frombuffer(b, dtype=np.uint8)
        parts.append(corpus.Corpus(np.concatenate([a, np.zeros(16, np.uint8)]),
                                   np.zeros(1, np.uint64), np.array([len(b)], np.uint32)))
    c = corpus.concat(*parts)
    raw = batch.upload(c)
    comp = batch.encode_slots(raw)
    batch.encode(raw, comp)
    torch.cuda.synchronize()
    return batch.to_host(comp).blocks()
