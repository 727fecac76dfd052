"""The encoder's batch after a copy (lgs_encode.hip, encode_pass, post_batch):
while the copy ended at least 125 bytes before the chunk's end every lane of
that batch is a probe and no validity is computed; past that bound the lanes
that are no probes swap with an empty mask and may put back what they read.
Lane B's upper bytes (snappy.c:182's 64-bit compare) come from lane 5's probe
word, not from a third probe dword.

The blocks of tests/test_gpu_encode_round.py end 20-24 bytes after their event,
so every batch of theirs is past that bound.  The blocks here
(encode_interior_cases.py) put the same events in the interior and on the
bound, one byte either side: lane B's re-match and its rejections, with the
search matching in the same batch or a later one; copies that end at and near
the chunk's end from an all-lanes round; matches at chosen lanes whose later
lanes swapped entries a following search needs; the 64-op flush with a long
tail behind it; token soup over the table-size steps and both LDS image
classes.  Each goes through the host batch, the device batch (1, 2 and 65
blocks a launch) and the drop-in, byte for byte against the reference encoder,
and round-trips through the reference decoder.

Every lane-B event stands at d = at - (n - 125) = -3 ... +3 and well inside,
with two exceptions that the parse itself sets.  The search's probe k is made
only while its next probe is inside the limit, OFFS[k + 1] <= 109 - d, so a
match at probe 62, 63 or 124 (from the second or third batch) exists only for
d <= -4, -8 and -744: those cases (b_rej_late*) stand at that largest d, one
byte further in, and well inside, and b_rej_nomatch_d-3 ... d+3 hold what there
is on the bound instead, B rejected and the search running out.  Likewise
probe 61 (lane 63) is on only for d <= 0: b_rej_search61_d+1 ... d+3 place the
repeat where that probe would stand and must find no match.

test_cases_are_what_they_say needs no GPU: it holds the Python restatement of
the parse to the reference's stream for every block, then asserts from it that
every block has the event, and stands on the side of the bound, its name says.
"""
from __future__ import annotations

import re

import pytest

import oracle
from encode_helpers import _copy_ops, _device_batch
from encode_interior_cases import INSIDE, INTERIOR, cases, parse, pieces

CASES = cases()
NAMES = [c.name for c in CASES]


@pytest.fixture(scope="module")
def expected():
    """The reference's bytes for every case, computed once."""
    ref = oracle.best()
    exp = {c.name: ref.encode(c.block) for c in CASES}
    for c in CASES:
        assert ref.decode(exp[c.name]) == c.block, c.name
    return exp


def test_cases_are_what_they_say(expected):
    assert 150 <= len(CASES) <= 400
    for c in CASES:
        copies, batches = parse(c.block)
        # the restatement against the reference, before anything it reports is used
        assert pieces(copies) == _copy_ops(expected[c.name]), c.name
        assert c.holds(), c.name
        assert len(c.block) <= 4608 or c.name in ("soup4609", "soup16896"), c.name
        # the side of the bound in the name is the block's
        m = re.search(r"_d([+-]\d+)$", c.name)
        if m:
            assert c.d == int(m.group(1)), (c.name, c.d)
        elif c.name.endswith("_inside"):
            assert c.d <= INSIDE, (c.name, c.d)
    by = {c.name: c for c in CASES}
    # both rounds, one byte either side of the bound, for every lane-B event
    for ev in ("b_rematch", "b4_nz0", "b4_nz1", "b4_nz2", "b_rej_search0", "b_rej_search1",
               "b_rej_search30", "b_rej_search61", "ab_share_rematch", "ab_share_rej", "only_a",
               "b_rej_nomatch"):
        for d in (-3, -2, -1, 0, 1, 2, 3):
            c = by[f"{ev}_d{d:+d}"]
            assert (c.at <= len(c.block) - INTERIOR) == (d <= 0), c.name
        assert by[f"{ev}_inside"].at + 300 <= len(by[f"{ev}_inside"].block) - INTERIOR
    # lane 63 (the search's probe 61) is on exactly in the all-lanes round
    for d in (-3, -2, -1, 0, 1, 2, 3):
        r = next(r for r in parse(by[f"b_rej_search61_d{d:+d}"].block)[1]
                 if r["at"] == by[f"b_rej_search61_d{d:+d}"].at)
        assert (r["probe"] == 61) == (d <= 0), (d, r)
    # copies from an all-lanes round that end at n - t, and the windows on the chunk's end
    for t in range(21):
        c = by[f"ext_end_t{t}"]
        base, ln, _ = parse(c.block)[0][-1]
        assert base + ln == len(c.block) - t and c.d <= 0, c.name
    for e in (63, 64, 65, 127, 128, 129):
        c = by[f"ext_edge{e}"]
        base, ln, _ = parse(c.block)[0][-1]
        assert len(c.block) - (base + 4) == e and base + ln == len(c.block) and c.d <= 0, c.name


def _check(outs, names, expected, route):
    ref = oracle.best()
    by = dict(zip(NAMES, CASES))
    for name, o in zip(names, outs):
        assert o == expected[name], (route, name)
        assert ref.decode(o) == by[name].block, (route, name)


@pytest.mark.gpu
def test_interior_host_batch(gpu, expected):
    _check(gpu.encode_batch_host([c.block for c in CASES]), NAMES, expected, "host")


def _launches():
    """(label, case indices): every case in a device launch of its size class;
    1, 2 and 65 blocks a launch."""
    small = [i for i, c in enumerate(CASES) if len(c.block) <= 4608]
    mid = [i for i, c in enumerate(CASES) if len(c.block) > 4608]
    out = [("small1", small[:1]), ("small2", small[1:3])]
    rest = small[3:]
    for j in range(0, len(rest), 65):
        out.append((f"small65_{j // 65}", (rest[j:] + small)[:65]))
    out += [("mid1", mid[:1]), ("mid2", mid[:2]), ("mid65", (mid + small)[:65])]
    assert {i for _, idx in out for i in idx} == set(range(len(CASES)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("label", [lb for lb, _ in _launches()])
def test_interior_device_batch(gpu, expected, label):
    idx = dict(_launches())[label]
    names = [NAMES[i] for i in idx]
    _check(_device_batch([CASES[i].block for i in idx]), names, expected, label)


@pytest.mark.gpu
def test_interior_dropin(gpu, expected):
    # (the service kernel shares encode_pass)
    _check([gpu.encode(c.block) for c in CASES], NAMES, expected, "dropin")
