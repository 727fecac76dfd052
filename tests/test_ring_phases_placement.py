"""tools/ring_phases.py (no GPU): the placement table built from the words the
phase-stamp probe writes (HW_ID bits 15:0 and XCC_ID in bits 19:16 of word 9,
the mover's, and word 25, the walker's, of each pair's 64 out_len words)."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ring_phases  # noqa: E402


def where(xcc: int, se: int, cu: int, simd: int, slot: int) -> int:
    return slot | simd << 4 | cu << 8 | se << 13 | xcc << 16


def words(pairs) -> np.ndarray:
    """pairs: (mover place, walker place, mover life, trips)."""
    v = np.zeros((len(pairs), 64), dtype=np.int64)
    for k, (m, w, life, trips) in enumerate(pairs):
        v[k, 0], v[k, 8], v[k, 9] = life, trips, m
        v[k, 16], v[k, 24], v[k, 25] = life, trips, w
    return v


def test_classes_by_what_shares_the_movers_simd():
    a, b, c = where(0, 0, 0, 0, 0), where(0, 0, 0, 1, 0), where(0, 0, 0, 2, 0)
    a1, b1, c1 = a | 1, b | 1, c | 1
    other_xcc = where(1, 0, 0, 0, 0)        # same HW_ID as a, another XCC: another SIMD
    v = words([
        (a, b, 1000, 10),                   # mover on a: (1,1) once pair 2's walker is there
        (b1, a1, 1100, 10),                 # mover on b beside pair 1's walker: (1,1)
        (c, other_xcc, 2000, 12),           # movers of pairs 3 and 4 share c: (0,2)
        (c1, other_xcc | 1, 2100, 13),
    ])
    p = ring_phases.placement(v)
    assert p["simds"] == 4 and p["cus"] == 2
    assert p["per_simd_walkers_movers"] == {"(0,2)": 1, "(1,1)": 2, "(2,0)": 1}
    assert p["slots_sharing_a_simd"] == {"(0, 1)": 4}
    rows = {r["class"]: r for r in p["rows"]}
    assert rows["(1,1)"]["pairs"] == 2 and rows["(0,2)"]["pairs"] == 2
    assert rows["(0,2)"]["life_max"] == 2100 and rows["(0,2)"]["trips_max"] == 13
    assert rows["(1,1)"]["life_p50"] == 1050.0
    assert rows["(0,2)"]["in_slowest_decile"] == 1 and rows["(1,1)"]["in_slowest_decile"] == 0
    table = ring_phases.placement_table(p)
    assert "(0,2)" in table and "(1,1)" in table
