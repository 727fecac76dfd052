"""Batched point lookups on the C2-scale fillseq table
(tools/bench_table_build.py's entries: 2 359 296 of 24 + 100 bytes, 65 536
blocks of 4 KiB).

* device-resident: lgs_block_seek_dev for --queries uniformly drawn stored
  keys against the decoded data blocks (lgs_block_cut_dev + lgs_block_emit_dev
  leave them on the device), HIP events, median of --iters runs after two
  warm-ups; beside it lgs_hbm_copy_dev moving the decoded blocks' bytes once
  (what the lookups must touch at the least) in the same run, and the same
  seek on the table's index block alone;
* host: lgs_table_get_host on the .ldb image lgs_table_build_host wrote, host
  arrays in and out, wall clock around the call, for --queries and for 1 024
  keys, median of --iters after two warm-ups;
* yardstick for the whole call: lcdb's own ldb_table_internal_get loop on one
  core, timed by `tests/golden/make_get_golden.py --time` ON THE BUILD HOST (a
  different machine: no reference binary runs here) and passed in with
  --ref-json; reported beside ours with that caveat.

* --open: the opened-table legs instead (lgs_table_open_host, lgs_table_get,
  lgs_table_get_dev, and lgs_table_get_host and the index block's
  lgs_table_read_host re-measured beside them), to
  profiles/table_get_open.json.

Writes one JSON object to --out (default profiles/table_get.json) and prints
it.  usage: python tools/bench_table_get.py [--entries N] [--queries Q] [--open]
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


def open_legs(a, L, check, e, np, torch) -> dict:
    """The opened-table legs (--open) on the same table image and key sets:
    lgs_table_open_host (borrowed and resident), lgs_table_get and
    lgs_table_get_dev for 1 024 and --queries keys, and beside them, in the
    same run, lgs_table_get_host and lgs_table_read_host of the index block
    alone.  Host calls by wall clock, lgs_table_get_dev by HIP events; median,
    minimum and maximum of --iters runs after two warm-ups."""
    from bench_table_build import host_build
    n, nq, bs = a.entries, a.queries, a.block_size
    keys = e[0]
    rng = np.random.default_rng(20240611)
    pick = rng.integers(0, n, size=nq)
    qkeys = np.concatenate([keys[:24 * n].reshape(n, 24)[pick].reshape(-1),
                            np.zeros(16, dtype=np.uint8)])
    qoff = np.arange(nq, dtype=np.uint64) * 24
    qlen = np.full(nq, 24, dtype=np.uint32)
    _, img = host_build(L, check, e, n, bs)
    img = np.concatenate([img, np.zeros(1, dtype=np.uint8)])
    flen = len(img) - 1
    small = min(1024, nq)
    out = {"workload": f"fillseq, {n} entries of 24 + 100 bytes, block_size {bs}; "
                       f"{nq} uniformly drawn stored keys", "entries": n, "queries": nq,
           "file_size": flen, "iters": a.iters}
    good = True

    def stats(ts):
        return {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3,
                "max_ms": max(ts) * 1e3}

    def wall(fn, after=None):
        ts = []
        for k in range(a.iters + 2):
            t0 = time.perf_counter()
            r = fn()
            t1 = time.perf_counter()
            if after:
                after(r)
            if k >= 2:
                ts.append(t1 - t0)
        return stats(ts)

    class Res:
        def __init__(self, m):
            self.called = np.zeros(m, dtype=np.uint8)
            self.status = np.zeros(m, dtype=np.uint8)
            self.verdict = np.zeros(m, dtype=np.uint8)
            self.cap = 124 * m
            self.out = np.empty(self.cap, dtype=np.uint8)
            self.ko = np.zeros(m + 1, dtype=np.uint64)
            self.vo = np.zeros(m + 1, dtype=np.uint64)
            self.need = C.c_size_t(0)

        def good(self):
            return bool(self.called.all()) and bool((self.status == 1).all()) and \
                bool((self.verdict == 1).all()) and self.need.value == self.cap

    # ---- the unchanged path, re-measured ----
    for m, name in ((nq, "get_host"), (small, "get_host_1024")):
        r = Res(m)
        out[name] = wall(lambda: check(L.lgs_table_get_host(
            img.ctypes.data, flen, 1, 0, 1, None, qkeys.ctypes.data, qoff.ctypes.data,
            qlen.ctypes.data, m, r.called.ctypes.data, r.status.ctypes.data, r.verdict.ctypes.data,
            r.out.ctypes.data, r.cap, r.ko.ctypes.data, r.vo.ctypes.data, C.byref(r.need)),
            "lgs_table_get_host"))
        good &= r.good()
    foot = img[flen - 48:flen].tobytes()
    at, hs = 0, []
    for _ in range(4):
        v, sh = 0, 0
        while True:
            c = foot[at]
            at += 1
            v |= (c & 127) << sh
            sh += 7
            if c < 128:
                break
        hs.append(v)
    hoff, hsize = np.array([hs[2]], dtype=np.uint64), np.array([hs[3]], dtype=np.uint64)
    icap = np.array([16 << 20], dtype=np.uint32)
    iout = np.empty(int(icap[0]) + 16, dtype=np.uint8)
    ioo, iol, ist = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
    out["read_host_index_block"] = wall(lambda: check(L.lgs_table_read_host(
        img.ctypes.data, flen, hoff.ctypes.data, hsize.ctypes.data, 1, 0, iout.ctypes.data,
        ioo.ctypes.data, icap.ctypes.data, iol.ctypes.data, ist.ctypes.data), "lgs_table_read_host"))
    good &= int(ist[0]) == 1
    out["index_block_bytes"] = int(iol[0])
    out["index_block_stored_bytes"] = int(hs[3])

    # ---- open, get, get_dev ----
    dq = torch.from_numpy(qkeys).cuda()
    dqo = torch.from_numpy(qoff.view(np.int64)).cuda()
    dql = torch.from_numpy(qlen.view(np.int32)).cuda()
    for resident, mode in ((0, "borrowed"), (1, "resident")):
        h, st = C.c_void_p(None), C.c_uint8(0)

        def opn():
            hh = C.c_void_p(None)
            check(L.lgs_table_open_host(img.ctypes.data, flen, 0, 1, None, resident, C.byref(hh),
                                        C.byref(st)), "lgs_table_open_host")
            return hh

        out[f"open_{mode}"] = wall(opn, after=L.lgs_table_close)
        h = opn()
        good &= st.value == 1
        ib, db = C.c_uint64(0), C.c_uint64(0)
        check(L.lgs_table_info(h, None, None, C.byref(ib), None, C.byref(db)), "lgs_table_info")
        out[f"device_bytes_{mode}"] = db.value
        good &= ib.value == out["index_block_bytes"]
        for m, name in ((nq, "get"), (small, "get_1024")):
            r = Res(m)
            out[f"{name}_{mode}"] = wall(lambda: check(L.lgs_table_get(
                h, 1, qkeys.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, m, r.called.ctypes.data,
                r.status.ctypes.data, r.verdict.ctypes.data, r.out.ctypes.data, r.cap,
                r.ko.ctypes.data, r.vo.ctypes.data, C.byref(r.need)), "lgs_table_get"))
            good &= r.good()
        if resident:
            for m, name in ((nq, "get_dev"), (small, "get_dev_1024")):
                u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda")   # noqa: E731
                called, status, verdict, res = u8(m), u8(m), u8(m), u8(124 * m)
                ko = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
                vo = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
                need = C.c_size_t(0)
                sp = torch.cuda.current_stream().cuda_stream
                ts = []
                for k in range(a.iters + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    check(L.lgs_table_get_dev(h, 1, dq.data_ptr(), dqo.data_ptr(), dql.data_ptr(), m,
                                              called.data_ptr(), status.data_ptr(), verdict.data_ptr(),
                                              res.data_ptr(), 124 * m, ko.data_ptr(), vo.data_ptr(),
                                              C.byref(need), sp), "lgs_table_get_dev")
                    e1.record()
                    torch.cuda.synchronize()
                    if k >= 2:
                        ts.append(e0.elapsed_time(e1) / 1e3)
                out[name] = stats(ts)
                good &= bool(called.all()) and bool((status == 1).all()) and \
                    bool((verdict == 1).all()) and need.value == 124 * m
        L.lgs_table_close(h)
    out["all_found"] = bool(good)
    # What the design predicts, as this run has it.
    out["get_1024_under_index_block_read"] = {
        mode: out[f"get_1024_{mode}"]["median_ms"] < out["read_host_index_block"]["median_ms"]
        for mode in ("borrowed", "resident")}
    out["get_not_slower_than_get_host"] = {
        mode: out[f"get_{mode}"]["median_ms"] <= out["get_host"]["max_ms"]
        for mode in ("borrowed", "resident")}
    return out


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--open", action="store_true",
                   help="the opened-table legs only, to profiles/table_get_open.json")
    p.add_argument("--entries", type=int, default=65536 * 36)
    p.add_argument("--queries", type=int, default=1 << 20)
    p.add_argument("--block-size", type=int, default=4096)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--ref-json", default=os.path.join(ROOT, "profiles", "table_get_reference.json"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_get.json"))
    a = p.parse_args()

    import numpy as np
    import torch

    from bench_table_build import fillseq_entries, host_build
    from lcdb_amd import _native, table
    from lcdb_amd._native import check
    L = _native.lib()
    if L.lgs_device_count() <= 0:
        sys.exit("bench_table_get: no GPU visible")
    torch.cuda.set_device(0)
    n, nq, bs = a.entries, a.queries, a.block_size
    e = fillseq_entries(n)
    keys = e[0]
    if a.open:
        out = open_legs(a, L, check, e, np, torch)
        path = a.out if a.out != p.get_default("out") else \
            os.path.join(ROOT, "profiles", "table_get_open.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(out))
        if not out["all_found"]:
            sys.exit(1)
        return
    out = {"workload": f"fillseq, {n} entries of 24 + 100 bytes, block_size {bs}; "
                       f"{nq} uniformly drawn stored keys", "entries": n, "queries": nq}

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
        return float(np.median(ts))

    def dev(x):
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                                x.view(np.int32) if x.dtype == np.uint32 else x).cuda()

    # ---- the decoded data blocks, resident ----
    d = [dev(x) for x in e]
    b = table.build_blocks(*d, block_size=bs, restart_interval=16, internal_keys=True)
    torch.cuda.synchronize()
    nb, raw_total = b["nblocks"], b["raw_total"]
    first = b["block_first"].cpu().numpy().astype(np.int64)
    rng = np.random.default_rng(20240611)
    pick = rng.integers(0, n, size=nq)
    qkeys = np.concatenate([keys[:24 * n].reshape(n, 24)[pick].reshape(-1),
                            np.zeros(16, dtype=np.uint8)])
    qoff = np.arange(nq, dtype=np.uint64) * 24
    qlen = np.full(nq, 24, dtype=np.uint32)
    qblock = (np.searchsorted(first, pick, side="right") - 1).astype(np.uint32)
    dq, dqo, dql, dqb = dev(qkeys), dev(qoff), dev(qlen), dev(qblock)
    i32 = lambda: torch.empty(nq, dtype=torch.int32, device="cuda")   # noqa: E731
    pos, fkl, vpos, vlen = i32(), i32(), i32(), i32()
    st = torch.empty(nq, dtype=torch.uint8, device="cuda")
    scr = torch.empty(int(L.lgs_block_seek_scratch(nq)), dtype=torch.uint8, device="cuda")

    def seek(blocks, boff, blen, nblocks, qb):
        check(L.lgs_block_seek_dev(blocks.data_ptr(), boff.data_ptr(), blen.data_ptr(), None,
                                   nblocks, qb.data_ptr(), dq.data_ptr(), dqo.data_ptr(),
                                   dql.data_ptr(), nq, 1, pos.data_ptr(), fkl.data_ptr(),
                                   vpos.data_ptr(), vlen.data_ptr(), st.data_ptr(), None, None,
                                   None, scr.data_ptr(), scr.numel(), None), "lgs_block_seek_dev")

    t_seek = timed(lambda: seek(b["raw"], b["raw_off"], b["raw_len"], nb, dqb))
    ok = bool((st == 1).all()) and bool((fkl == 24).all()) and bool((vlen == 100).all())
    half = (raw_total // 2 + 15) // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    t_copy = timed(lambda: check(L.lgs_hbm_copy_dev(dst.data_ptr(), src.data_ptr(), half, None),
                                 "lgs_hbm_copy_dev"))
    copy_rate = 2 * half / t_copy
    out.update({
        "blocks": nb, "raw_bytes": raw_total,
        "block_seek_ms": t_seek * 1e3, "block_seek_all_found": ok,
        "block_seek_ns_per_query": t_seek / nq * 1e9,
        "hbm_copy_GBps": copy_rate / 1e9,
        "floor_ms_blocks_once_at_copy_rate": raw_total / copy_rate * 1e3,
        "block_seek_over_floor": t_seek / (raw_total / copy_rate),
        "budget_ms": [0.2, 0.4],
    })
    del src, dst

    # ---- the host call on the table image ----
    _, img = host_build(L, check, e, n, bs)
    img = np.concatenate([img, np.zeros(1, dtype=np.uint8)])
    flen = len(img) - 1

    # The same seek on the index block alone (restart interval 1, one block).
    handles, _, _, ist = table.index_host(img[:flen].tobytes(), internal_keys=True, filter_name=None)
    foot = img[flen - 48:flen].tobytes()
    at, hs = 0, []
    for _ in range(4):
        v, sh = 0, 0
        while True:
            c = foot[at]
            at += 1
            v |= (c & 127) << sh
            sh += 7
            if c < 128:
                break
        hs.append(v)
    (index,), _ = table.read_blocks_host(img[:flen], [hs[2]], [hs[3]], [16 << 20], verify=False)
    di = dev(np.frombuffer(index + b"\0" * 16, dtype=np.uint8).copy())
    zo = torch.zeros(1, dtype=torch.int64, device="cuda")
    il = torch.full((1,), len(index), dtype=torch.int32, device="cuda")
    zb = torch.zeros(nq, dtype=torch.int32, device="cuda")
    t_index = timed(lambda: seek(di, zo, il, 1, zb))
    out.update({"index_block_bytes": len(index), "index_seek_ms": t_index * 1e3,
                "index_seek_all_found": bool((st == 1).all()) and bool((pos != -1).all())})

    def host_get(m):
        called = np.zeros(m, dtype=np.uint8)
        status = np.zeros(m, dtype=np.uint8)
        verdict = np.zeros(m, dtype=np.uint8)
        cap = 124 * m
        res = np.empty(cap, dtype=np.uint8)
        ko = np.zeros(m + 1, dtype=np.uint64)
        vo = np.zeros(m + 1, dtype=np.uint64)
        need = C.c_size_t(0)
        ts = []
        for k in range(a.iters + 2):
            t0 = time.perf_counter()
            check(L.lgs_table_get_host(img.ctypes.data, flen, 1, 0, 1, None, qkeys.ctypes.data,
                                       qoff.ctypes.data, qlen.ctypes.data, m, called.ctypes.data,
                                       status.ctypes.data, verdict.ctypes.data, res.ctypes.data, cap,
                                       ko.ctypes.data, vo.ctypes.data, C.byref(need)),
                  "lgs_table_get_host")
            if k >= 2:
                ts.append(time.perf_counter() - t0)
        good = bool(called.all()) and bool((status == 1).all()) and bool((verdict == 1).all()) \
            and need.value == cap
        return float(np.median(ts)), good

    t_big, ok_big = host_get(nq)
    t_small, ok_small = host_get(min(1024, nq))
    out.update({"get_host_ms": t_big * 1e3, "get_host_ns_per_lookup": t_big / nq * 1e9,
                "get_host_all_found": ok_big, "get_host_1024_ms": t_small * 1e3,
                "get_host_1024_us_per_lookup": t_small / min(1024, nq) * 1e6,
                "get_host_1024_all_found": ok_small, "file_size": flen})

    if os.path.exists(a.ref_json):
        with open(a.ref_json) as f:
            ref = json.load(f)
        out["reference_one_core_OTHER_HOST"] = ref
        if ref.get("ns_per_lookup"):
            out["get_host_vs_reference_one_core_other_host"] = \
                ref["ns_per_lookup"] / (t_big / nq * 1e9)
            out["get_host_1024_vs_reference_one_core_other_host"] = \
                ref["ns_per_lookup"] / (t_small / min(1024, nq) * 1e9)
    else:
        out["reference_one_core_OTHER_HOST"] = "not measured"

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))
    if not (ok and ok_big and ok_small):
        sys.exit(1)


if __name__ == "__main__":
    main()
