"""Merging sorted runs on runs of the fill4096_internal shape:
fillseq entries (a 16-digit decimal user key + tag, 100-byte values;
tools/bench_table_build.py's) dealt round-robin into k = 4 and k = 12 runs, so
the runs overlap over the whole key space; about 10^6 entries in all, resident
on the device.

* lgs_merge_plan_dev and lgs_merge_emit_dev, each call and the pair, by HIP
  events (median, minimum and maximum of --iters runs after two warm-ups);
  ns per entry and GiB/s of entry bytes (keys + values read once);
* the same with the drop rule on (smallest_snapshot in the middle of the
  sequences, drop_deletions = 0: nothing is a deletion, so rule (A) never
  fires across distinct user keys and every entry is kept -- the rule's cost
  alone);
* beside them lgs_hbm_copy_dev moving the entry bytes once in and once out
  (the floor of the emit);
* the result checked: the merged order is the entries the runs were dealt
  from, src_run / src_index name the deal.

The per-kernel split comes from a separate run under `rocprofv3
--kernel-trace --stats` with --iters 3.  The yardstick is lcdb's own merging
loop on one core, timed by `tests/golden/make_merge_golden.py --time-deal K N
REPS` ON THE BUILD HOST (a different machine: no reference binary runs here)
and read from --ref-json; reported beside ours with that caveat.

Writes one JSON object to --out (default profiles/merge.json) and prints it.
usage: python tools/bench_merge.py [--entries N] [--runs 4,12]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def deal_runs(e, n: int, k: int):
    """Run r = entries r, r + k, ... of fillseq_entries' arrays, as numpy
    arrays in the run layout (offsets with n + 1 values)."""
    import numpy as np
    keys = e[0][:24 * n].reshape(n, 24)
    vals = e[3][:100 * n].reshape(n, 100)
    pad = np.zeros(16, dtype=np.uint8)
    runs = []
    for r in range(k):
        m = len(range(r, n, k))
        runs.append((np.concatenate([keys[r::k].reshape(-1), pad]),
                     np.arange(m + 1, dtype=np.uint64) * 24, np.full(m, 24, dtype=np.uint32),
                     np.concatenate([vals[r::k].reshape(-1), pad]),
                     np.arange(m + 1, dtype=np.uint64) * 100, np.full(m, 100, dtype=np.uint32), m))
    return runs


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--entries", type=int, default=1 << 20)
    p.add_argument("--runs", default="4,12")
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--ref-json", default=os.path.join(ROOT, "profiles", "merge_reference.json"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge.json"))
    a = p.parse_args()

    import numpy as np
    import torch

    from bench_table_build import fillseq_entries
    from lcdb_amd import _native
    from lcdb_amd._native import check
    L = _native.lib()
    if L.lgs_device_count() <= 0:
        sys.exit("bench_merge: no GPU visible")
    torch.cuda.set_device(0)
    n = a.entries
    e = fillseq_entries(n)
    kb, vb = 24 * n, 100 * n
    out = {"workload": f"fillseq, {n} entries of 24 + 100 bytes dealt round-robin", "entries": n,
           "iters": a.iters, "entry_bytes": kb + vb}

    def stats(ts):
        return {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3,
                "max_ms": max(ts) * 1e3}

    def timed(fn):
        ts = []
        for k in range(a.iters + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= 2:
                ts.append(e0.elapsed_time(e1) / 1e3)
        return stats(ts)

    def dev(x):
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                                x.view(np.int32) if x.dtype == np.uint32 else x).cuda()

    want_keys, want_vals = dev(e[0][:kb]), dev(e[3][:vb])
    keys = torch.zeros(kb + 16, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(vb + 16, dtype=torch.uint8, device="cuda")
    koff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    voff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    klen, vlen, srun, sidx = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4))
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")

    half = ((kb + vb) + 15) // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    t_copy = timed(lambda: check(L.lgs_hbm_copy_dev(dst.data_ptr(), src.data_ptr(), half, None),
                                 "lgs_hbm_copy_dev"))
    rate = 2 * half / (t_copy["median_ms"] / 1e3)
    out["hbm_copy_GBps"] = rate / 1e9
    out["emit_floor_ms_at_copy_rate"] = 2 * (kb + vb) / rate * 1e3
    del src, dst

    ok_all = True
    for k in (int(x) for x in a.runs.split(",")):
        host = deal_runs(e, n, k)
        held = [[dev(x) for x in r[:6]] for r in host]
        arr = (_native.LgsRun * k)()
        for r in range(k):
            arr[r] = _native.LgsRun(*(t.data_ptr() for t in held[r]), host[r][6])
        scr = torch.empty(int(L.lgs_merge_scratch(n, k)), dtype=torch.uint8, device="cuda")
        res = {"runs": k, "scratch_bytes": int(scr.numel())}

        def plan(drop=0, snap=0):
            check(L.lgs_merge_plan_dev(arr, k, 1, drop, snap, 0, counts.data_ptr(), scr.data_ptr(),
                                       scr.numel(), None), "lgs_merge_plan_dev")

        def emit():
            check(L.lgs_merge_emit_dev(arr, k, n, keys.data_ptr(), koff.data_ptr(),
                                       klen.data_ptr(), vals.data_ptr(), voff.data_ptr(),
                                       vlen.data_ptr(), srun.data_ptr(), sidx.data_ptr(),
                                       scr.data_ptr(), scr.numel(), None), "lgs_merge_emit_dev")

        res["plan"] = timed(plan)
        got = [int(x) for x in counts.cpu()]
        res["emit"] = timed(emit)
        res["plan_emit"] = timed(lambda: (plan(), emit()))
        res["plan_emit_drop_rule"] = timed(lambda: (plan(1, n // 2), emit()))
        plan()
        emit()
        torch.cuda.synchronize()
        i = torch.arange(n, device="cuda")
        ok = (got[:6] == [n, kb, vb, 24, 0, -1] and
              bool((keys[:kb] == want_keys).all()) and bool((vals[:vb] == want_vals).all()) and
              bool((klen == 24).all()) and bool((vlen == 100).all()) and
              int(koff[n]) == kb and int(voff[n]) == vb and
              bool((srun == (i % k).to(torch.int32)).all()) and
              bool((sidx == (i // k).to(torch.int32)).all()))
        res["equals_the_dealt_entries"] = bool(ok)
        ok_all = ok_all and ok
        ms = res["plan_emit"]["median_ms"]
        res["ns_per_entry"] = ms * 1e6 / n
        res["entry_GiBps"] = (kb + vb) / (ms / 1e3) / 2 ** 30
        res["emit_over_floor"] = res["emit"]["median_ms"] / out["emit_floor_ms_at_copy_rate"]
        out[f"k{k}"] = res
        del scr, held

    if os.path.exists(a.ref_json):
        with open(a.ref_json) as f:
            out["reference_one_core_OTHER_HOST"] = json.load(f)
    else:
        out["reference_one_core_OTHER_HOST"] = "not measured"

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
