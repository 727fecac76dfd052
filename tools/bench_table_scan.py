"""Forward scans on the C2-scale fillseq table
(tools/bench_table_build.py's entries: 2 359 296 of 24 + 100 bytes, 65 536
blocks of 4 KiB).

* lgs_block_entries_count_dev + lgs_block_entries_emit_dev on the resident
  decoded blocks (lgs_block_cut_dev + lgs_block_emit_dev leave them on the
  device), each call and the pair by HIP events;
* lgs_table_scan_dev of the whole table opened resident (Snappy blocks,
  checksums verified), by HIP events;
* lgs_table_scan of the same table opened borrowed, into host memory, by wall
  clock;
* beside them, in the same run, lgs_hbm_copy_dev moving the bytes the block
  scan reads plus writes (the floor), DESIGN §4.7's budget, and the first
  scan's extra time for the index entry list.

Median, minimum and maximum of --iters runs after two warm-ups.  The
yardstick for the whole scan is lcdb's own iterator loop on one core, timed by
`tests/golden/make_scan_golden.py --time` ON THE BUILD HOST (a different
machine: no reference binary runs here) and read from --ref-json; reported
beside ours with that caveat.  The output is checked against the entries the
table was built from.

Writes one JSON object to --out (default profiles/table_scan.json) and prints
it.  usage: python tools/bench_table_scan.py [--entries N]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BUDGET_MS = {"block_entries": [0.8, 1.3], "table_scan_dev": [1.6, 2.2],
             "table_scan_host": [50, 100]}


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--entries", type=int, default=65536 * 36)
    p.add_argument("--block-size", type=int, default=4096)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--ref-json", default=os.path.join(ROOT, "profiles", "table_scan_reference.json"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_scan.json"))
    a = p.parse_args()

    import numpy as np
    import torch

    from bench_table_build import fillseq_entries, host_build
    from lcdb_amd import _native, table
    from lcdb_amd._native import check
    L = _native.lib()
    if L.lgs_device_count() <= 0:
        sys.exit("bench_table_scan: no GPU visible")
    torch.cuda.set_device(0)
    n, bs = a.entries, a.block_size
    e = fillseq_entries(n)
    kb, vb = 24 * n, 100 * n
    out = {"workload": f"fillseq, {n} entries of 24 + 100 bytes, block_size {bs}", "entries": n,
           "iters": a.iters, "budget_ms": BUDGET_MS}

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

    def same(keys, koff, klen, vals, voff, vlen, m):
        return (m == n and bool((keys[:kb] == want_keys).all()) and
                bool((vals[:vb] == want_vals).all()) and
                bool((klen[:n] == 24).all()) and bool((vlen[:n] == 100).all()) and
                int(koff[n]) == kb and int(voff[n]) == vb)

    # ---- the decoded data blocks, resident ----
    d = [dev(x) for x in e]
    b = table.build_blocks(*d, block_size=bs, restart_interval=16, internal_keys=True)
    torch.cuda.synchronize()
    nb, raw_total = b["nblocks"], b["raw_total"]
    del d
    scr = torch.empty(int(L.lgs_block_entries_scratch(nb, raw_total)), dtype=torch.uint8,
                      device="cuda")
    first = torch.zeros(nb + 1, dtype=torch.int32, device="cuda")
    bst = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    keys = torch.zeros(kb + 16, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(vb + 16, dtype=torch.uint8, device="cuda")
    koff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    voff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    klen = torch.zeros(n, dtype=torch.int32, device="cuda")
    vlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    head = (b["raw"].data_ptr(), b["raw_off"].data_ptr(), b["raw_len"].data_ptr(), None, nb,
            raw_total, None, None, 1)

    def count():
        check(L.lgs_block_entries_count_dev(*head, first.data_ptr(), bst.data_ptr(),
                                            counts.data_ptr(), scr.data_ptr(), scr.numel(), None),
              "lgs_block_entries_count_dev")

    def emit():
        check(L.lgs_block_entries_emit_dev(*head, n, keys.data_ptr(), koff.data_ptr(),
                                           klen.data_ptr(), vals.data_ptr(), voff.data_ptr(),
                                           vlen.data_ptr(), scr.data_ptr(), scr.numel(), None),
              "lgs_block_entries_emit_dev")

    out["block_entries_count"] = timed(count)
    got = [int(x) for x in counts.cpu()]
    out["block_entries_emit"] = timed(emit)
    out["block_entries"] = timed(lambda: (count(), emit()))
    ok_blocks = got == [n, kb, vb, 24] and bool((bst == 1).all()) and \
        same(keys, koff, klen, vals, voff, vlen, got[0])
    # The floor: the bytes the pair must read (the blocks, once) and write
    # (keys, values, offsets, lengths), moved once at the copy kernel's rate.
    moved = raw_total + kb + vb + 24 * n
    half = (moved // 2 + 15) // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    t_copy = timed(lambda: check(L.lgs_hbm_copy_dev(dst.data_ptr(), src.data_ptr(), half, None),
                                 "lgs_hbm_copy_dev"))
    rate = 2 * half / (t_copy["median_ms"] / 1e3)
    del src, dst
    out.update({"blocks": nb, "raw_bytes": raw_total, "scratch_bytes": int(scr.numel()),
                "bytes_read_plus_written": moved, "hbm_copy_GBps": rate / 1e9,
                "floor_ms_at_copy_rate": moved / rate * 1e3,
                "block_entries_over_floor": out["block_entries"]["median_ms"] /
                (moved / rate * 1e3), "block_entries_equal_the_input": bool(ok_blocks)})
    del scr, b

    # ---- the whole table ----
    _, img = host_build(L, check, e, n, bs)
    img = np.ascontiguousarray(img)
    out["file_size"] = len(img)
    cap_blocks = nb + 16
    dfirst = torch.zeros(cap_blocks + 1, dtype=torch.int32, device="cuda")
    dbst = torch.zeros(cap_blocks, dtype=torch.uint8, device="cuda")
    done, nxt, at_end = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
    ist = C.c_uint8(0)
    needed = np.zeros(4, dtype=np.uint64)
    sp = torch.cuda.current_stream().cuda_stream

    def scan_dev(t):
        check(L.lgs_table_scan_dev(t._handle(), 1, None, 0, 0, 0, cap_blocks, keys.data_ptr(),
                                   kb + 16, koff.data_ptr(), klen.data_ptr(), vals.data_ptr(),
                                   vb + 16, voff.data_ptr(), vlen.data_ptr(), n, dfirst.data_ptr(),
                                   dbst.data_ptr(), C.byref(done), C.byref(nxt), C.byref(at_end),
                                   C.byref(ist), needed.ctypes.data, sp), "lgs_table_scan_dev")

    with table.open_table(img, internal_keys=True, filter_name=None, resident=True) as t:
        before = t.info()["device_bytes"]
        keys.zero_()
        vals.zero_()
        t0 = time.perf_counter()
        scan_dev(t)
        torch.cuda.synchronize()
        t_first = time.perf_counter() - t0
        out["index_entry_list_bytes"] = t.info()["device_bytes"] - before
        ok_dev = done.value == nb and at_end.value == 1 and ist.value == 1 and \
            bool((dbst[:nb] == 1).all()) and same(keys, koff, klen, vals, voff, vlen, int(needed[0]))
        out["table_scan_dev"] = timed(lambda: scan_dev(t))
        ts = []
        for k in range(a.iters + 2):
            t0 = time.perf_counter()
            scan_dev(t)
            torch.cuda.synchronize()
            if k >= 2:
                ts.append(time.perf_counter() - t0)
        out["table_scan_dev_wall"] = stats(ts)
        out["first_scan_extra_ms"] = t_first * 1e3 - out["table_scan_dev_wall"]["median_ms"]
    out["table_scan_dev_equals_the_input"] = bool(ok_dev)
    out["table_scan_dev_over_floor"] = out["table_scan_dev"]["median_ms"] / (moved / rate * 1e3)

    hkeys = np.zeros(kb + 16, dtype=np.uint8)
    hvals = np.zeros(vb + 16, dtype=np.uint8)
    hkoff, hvoff = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    hklen, hvlen = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    hfirst, hbst = np.zeros(cap_blocks + 1, dtype=np.uint32), np.zeros(cap_blocks, dtype=np.uint8)

    with table.open_table(img, internal_keys=True, filter_name=None, resident=False) as t:
        ts = []
        for k in range(a.iters + 2):
            t0 = time.perf_counter()
            check(L.lgs_table_scan(t._handle(), 1, None, 0, 0, 0, cap_blocks, hkeys.ctypes.data, kb,
                                   hkoff.ctypes.data, hklen.ctypes.data, hvals.ctypes.data, vb,
                                   hvoff.ctypes.data, hvlen.ctypes.data, n, hfirst.ctypes.data,
                                   hbst.ctypes.data, C.byref(done), C.byref(nxt), C.byref(at_end),
                                   C.byref(ist), needed.ctypes.data), "lgs_table_scan")
            if k >= 2:
                ts.append(time.perf_counter() - t0)
        out["table_scan_host"] = stats(ts)
    ok_host = done.value == nb and at_end.value == 1 and ist.value == 1 and \
        bool((hbst[:nb] == 1).all()) and int(needed[0]) == n and \
        bool((hkeys[:kb] == e[0][:kb]).all()) and bool((hvals[:vb] == e[3][:vb]).all()) and \
        bool((hklen == 24).all()) and bool((hvlen == 100).all())
    out["table_scan_host_equals_the_input"] = bool(ok_host)
    out["table_scan_host_ns_per_entry"] = out["table_scan_host"]["median_ms"] * 1e6 / n

    if os.path.exists(a.ref_json):
        with open(a.ref_json) as f:
            ref = json.load(f)
        out["reference_one_core_OTHER_HOST"] = ref
        if ref.get("ns_per_scan"):
            out["table_scan_host_vs_reference_one_core_other_host"] = \
                ref["ns_per_scan"] / 1e6 / out["table_scan_host"]["median_ms"]
            out["table_scan_dev_vs_reference_one_core_other_host"] = \
                ref["ns_per_scan"] / 1e6 / out["table_scan_dev"]["median_ms"]
    else:
        out["reference_one_core_OTHER_HOST"] = "not measured"

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))
    if not (ok_blocks and ok_dev and ok_host):
        sys.exit(1)


if __name__ == "__main__":
    main()
