#!/usr/bin/env python3
"""Where a trip's cycles go in the lane-per-block decoders on C2, from a
probe build with -DLGS_PROBE_RING_PHASES (lgs_probe_hooks.h): each wave sums
the shader-clock cycles (s_memtime) of its trip phases.

decode_ring_kernel (probe library only, lgs_decode_ring.hip): lane k < 8 of
the wave writes phase k's sum into its block's out_len, lane 8 the trip count.

Phases: 0 first-slot piece (before the wait), 1 the trip's vmcnt(0),
2 far-copy and refill landing, 3 flush jobs, 4 first parse, 5 second slot
(piece + parse), 6 refill requests, 7 the loop test.  Each stamp is an
s_memtime whose use waits for every outstanding LDS operation too, so LDS
latency is charged to the phase whose operations are in flight at its end.

The "ring" route is decode_pair_kernel: its two roles stamp their own
phases (PAIR_MOVER, PAIR_WALKER below), the mover's lanes 0-8 and the
walker's lanes 16-24 of each 64-block workgroup write them.  With
LGS_DECODE_KERNEL=ring32 a probe build that also has -DLGS_PROBE_DECODERS and
the probe sources (build.PROBE_SOURCES; tools/mk_variants.sh adds them when
FLAGS hold -DLGS_PROBE_DECODERS) runs decode_ring_kernel and the layout above;
a build without them only warns that "ring32" names a probe-library decoder
and runs the pair kernel.

usage: python tools/ring_phases.py PROBE_SO [PRODUCT_SO]
Prints one JSON line: per-phase cycles per wave (median over waves), per
trip, the share of the wave's life, and the launch times of the probe and
(if given) the product library, HIP-event timed.  For the pair kernel a
table follows: mover life and trips by what else ran on the mover's SIMD
(lane 9 of the mover and lane 25 of the walker report HW_ID and XCC_ID).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["piece1", "wait_vmcnt", "landing", "flush", "parse1", "slot2", "refill_req", "loop_test"]
# decode_pair_kernel (the "ring" route; LGS_DECODE_KERNEL=ring32 selects the
# probe library's old kernel and the layout above): each role's phases 0-4, and 7 = from its
# last stamp through the barrier to the top of the next trip, i.e. mostly the
# wait for the other role.
PAIR_MOVER = ["wait_vmcnt", "far_landing", "flush", "slot1", "slot2", "", "", "barrier"]
PAIR_WALKER = ["wait_vmcnt", "refill_landing", "slot1", "slot2", "end_refill_req", "", "", "barrier"]


def placement(v) -> dict:
    """Life against placement: v is one row of 64 out_len words per
    walker/mover pair.  Word 9 (mover) and word 25 (walker) hold where the wave
    ran: HW_ID bits 15:0 (wave slot 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13)
    and the XCC id in bits 19:16.  A pair's class is the (walkers, movers)
    count of the SIMD its mover ran on."""
    import collections
    import numpy as np

    def simd(w):     # (xcc, se/sh/cu, simd): one id per SIMD of the chip
        return (w >> 16) * 4096 + ((w >> 8) & 0xff) * 4 + ((w >> 4) & 3)

    mw, ww = v[:, 9], v[:, 25]
    ms, ws = simd(mw), simd(ww)
    nm, nw = collections.Counter(ms.tolist()), collections.Counter(ws.tolist())
    per_simd = collections.Counter((nw.get(s, 0), nm.get(s, 0)) for s in set(nm) | set(nw))
    cls = np.array([nw.get(s, 0) * 10 + nm.get(s, 0) for s in ms.tolist()])
    life, trips = v[:, 0:8].sum(axis=1), v[:, 8]
    slow = life >= np.percentile(life, 90)
    rows = []
    for c in sorted(set(cls.tolist())):
        k = cls == c
        rows.append({"class": "(%d,%d)" % (c // 10, c % 10), "pairs": int(k.sum()),
                     "trips_p50": float(np.median(trips[k])), "trips_max": int(trips[k].max()),
                     "life_p50": float(np.median(life[k])),
                     "life_p90": float(np.percentile(life[k], 90)),
                     "life_max": int(life[k].max()),
                     "in_slowest_decile": int((k & slow).sum())})
    # The wave slots of two waves that share a SIMD (do their low bits differ?).
    by = collections.defaultdict(list)
    for s, w in zip(ms.tolist() + ws.tolist(), mw.tolist() + ww.tolist()):
        by[s].append(w & 15)
    slots = collections.Counter(tuple(sorted(x)) for x in by.values())
    return {"simds": len(by), "cus": len({s // 4 for s in by}),
            "per_simd_walkers_movers": {"(%d,%d)" % k: n for k, n in sorted(per_simd.items())},
            "slots_sharing_a_simd": {str(k): n for k, n in sorted(slots.items())},
            "slowest_decile_pairs": int(slow.sum()),
            "corr_life_trips": float(np.corrcoef(life, trips)[0, 1]),
            "rows": rows}


def placement_table(p: dict) -> str:
    out = ["# mover life by what shares the mover's SIMD, class = (walkers, movers) on it",
           "# SIMDs %d  CUs %d  per-SIMD (walkers, movers): %s" % (
               p["simds"], p["cus"], p["per_simd_walkers_movers"]),
           "# wave slots of the waves sharing a SIMD: %s" % p["slots_sharing_a_simd"],
           "# slowest decile: %d pairs; corr(life, trips) = %.3f" % (
               p["slowest_decile_pairs"], p["corr_life_trips"]),
           "class   pairs  trips_p50  trips_max   life_p50   life_p90   life_max  in_slowest_decile"]
    for r in p["rows"]:
        out.append("%-6s %6d %10.0f %10d %10.0f %10.0f %10d %10d" % (
            r["class"], r["pairs"], r["trips_p50"], r["trips_max"], r["life_p50"], r["life_p90"],
            r["life_max"], r["in_slowest_decile"]))
    return "\n".join(out)


def child(lib: str, phases: bool) -> dict:
    sys.path.insert(0, ROOT)
    import lcdb_amd.build as b
    b.LIB = os.path.abspath(lib)
    import numpy as np
    import torch
    from lcdb_amd import batch, corpus
    c = corpus.fillseq(65536)
    raw = batch.upload(c)
    comp = batch.encode_slots(raw)
    batch.encode(raw, comp)
    out = batch.decode_slots(c.len)
    st = torch.zeros(c.n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    ts = []
    for k in range(13):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        batch.decode(comp, out, st, s)
        e1.record(s)
        e1.synchronize()
        if k >= 3:
            ts.append(e0.elapsed_time(e1) * 1000.0)
    res = {"lib": os.path.basename(lib), "decode_us_p50": float(np.median(ts)),
           "status_ok": bool((st == 1).all())}
    if phases and os.environ.get("LGS_DECODE_KERNEL") != "ring32":
        # decode_pair_kernel: 64 blocks per workgroup; the mover's lanes 0-8
        # and the walker's lanes 16-24 hold their role's sums and trip count.
        v = out.len.cpu().numpy().astype(np.float64).reshape(-1, 64)
        res["workgroups"] = int(v.shape[0])
        for role, base, names in (("mover", 0, PAIR_MOVER), ("walker", 16, PAIR_WALKER)):
            ph, trips = v[:, base:base + 8], v[:, base + 8]
            med, t50 = np.median(ph, axis=0), float(np.median(trips))
            res[role] = {
                "trips_p50": t50, "life_cycles_p50": float(np.median(ph.sum(axis=1))),
                "life_cycles_max": float(ph.sum(axis=1).max()),
                "phase_cycles_per_trip": {n: round(float(x) / t50, 1)
                                          for n, x in zip(names, med) if n},
                "work_cycles_per_trip": round(float(med[:7].sum()) / t50, 1)}
        words = out.len.cpu().numpy().astype(np.int64).reshape(-1, 64)
        res["placement"] = placement(words)
        if os.environ.get("RING_PHASES_DUMP"):     # the raw words, for a closer look
            np.save(os.environ["RING_PHASES_DUMP"], words)
    elif phases:
        v = out.len.cpu().numpy().astype(np.float64).reshape(-1, 32)   # 32 blocks per wave
        ph = v[:, :8]
        trips = v[:, 8]
        life = ph.sum(axis=1)
        med = np.median(ph, axis=0)
        res["waves"] = int(v.shape[0])
        res["trips_p50"] = float(np.median(trips))
        res["life_cycles_p50"] = float(np.median(life))
        res["life_cycles_max"] = float(life.max())
        res["phase_cycles_per_wave_p50"] = {n: float(x) for n, x in zip(NAMES, med)}
        res["phase_cycles_per_trip"] = {n: round(float(x) / float(np.median(trips)), 1)
                                        for n, x in zip(NAMES, med)}
        res["phase_share"] = {n: round(float(x) / float(med.sum()), 3) for n, x in zip(NAMES, med)}
    return res


def main() -> None:
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        print(json.dumps(child(sys.argv[2], sys.argv[3] == "1")))
        return
    libs = [(sys.argv[1], "1")] + ([(sys.argv[2], "0")] if len(sys.argv) > 2 else [])
    out = {}
    for lib, ph in libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, ph],
                           capture_output=True, text=True, check=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        d = json.loads(line)
        out["probe" if ph == "1" else "product"] = d
    print(json.dumps(out))
    if "placement" in out.get("probe", {}):
        print(placement_table(out["probe"]["placement"]))


if __name__ == "__main__":
    main()
