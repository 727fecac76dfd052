"""Whole-table build from sorted entries: the device block
builder and lgs_table_build_host on db_bench fillseq entries (keys "%016d" as
internal keys with sequence k + 1, 100-byte values from the db_bench ring --
what oracle/harness/build_table.c feeds lcdb), beside the reference's own
block builder on one host core.

* device-resident: lgs_block_cut_dev and lgs_block_emit_dev, HIP events on
  the launch stream, median of --iters runs after two warm-ups; the emit's
  bytes (entries read + blocks written) over its time, against
  lgs_hbm_copy_dev moving the same number of bytes in the same run;
* host: build_table_host, wall clock around the call (it ends in a
  synchronisation), first call and median of the next three;
* yardstick: cut_s, write_warm_s and finish_s printed by
  oracle/_ref/lcdb/build_table_batched.gpu for the same entry count in the
  same run, and the SHA-256 of the file it wrote against ours;
* --c5: the 32 768 000-entry table, its SHA-256 against
  tests/golden/digests.json C5_table_2GiB.

Writes one JSON object to --out (default profiles/table_build.json) and
prints it.  usage: python tools/bench_table_build.py [--entries N] [--c5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fillseq_entries(n: int):
    """(keys, key_off, key_len, vals, val_off, val_len) numpy arrays."""
    import numpy as np

    from lcdb_amd import corpus
    keys = np.empty((n, 24), dtype=np.uint8)
    step = 1 << 20
    p10 = 10 ** np.arange(15, -1, -1, dtype=np.int64)
    for a in range(0, n, step):
        k = np.arange(a, min(n, a + step), dtype=np.int64)
        keys[a:a + len(k), :16] = (k[:, None] // p10 % 10 + 48).astype(np.uint8)
        tag = ((k + 1) << 8) | 1                                   # LDB_TYPE_VALUE
        keys[a:a + len(k), 16:] = tag.astype("<u8").view(np.uint8).reshape(-1, 8)
    ring = np.frombuffer(corpus.value_ring(), dtype=np.uint8)
    per = len(ring) // 100                       # the ring restarts when 100 bytes do not fit
    vals = np.resize(ring[:per * 100].reshape(per, 100), (n, 100))
    pad = np.zeros(16, dtype=np.uint8)
    return (np.concatenate([keys.reshape(-1), pad]), np.arange(n, dtype=np.uint64) * 24,
            np.full(n, 24, dtype=np.uint32), np.concatenate([vals.reshape(-1), pad]),
            np.arange(n, dtype=np.uint64) * 100, np.full(n, 100, dtype=np.uint32))


def host_build(L, check, e, n, block_size):
    import numpy as np
    keys, koff, klen, vals, voff, vlen = e
    cap = int(L.lgs_table_build_bound(n, 24 * n, 100 * n, 0))
    file = np.empty(cap, dtype=np.uint8)
    size = C.c_size_t(0)
    t0 = time.perf_counter()
    check(L.lgs_table_build_host(keys.ctypes.data, koff.ctypes.data, klen.ctypes.data,
                                 vals.ctypes.data, voff.ctypes.data, vlen.ctypes.data, n,
                                 block_size, 16, 1, 0, 1, file.ctypes.data, cap, C.byref(size)),
          "lgs_table_build_host")
    return time.perf_counter() - t0, file[:size.value]


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--entries", type=int, default=65536 * 36)
    p.add_argument("--block-size", type=int, default=4096)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--c5", action="store_true", help="also build the 32 768 000-entry table")
    p.add_argument("--no-ref", action="store_true", help="skip build_table_batched.gpu")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_build.json"))
    a = p.parse_args()

    import numpy as np
    import torch

    from lcdb_amd import _native
    from lcdb_amd._native import check
    L = _native.lib()
    if L.lgs_device_count() <= 0:
        sys.exit("bench_table_build: no GPU visible")
    torch.cuda.set_device(0)
    n, bs = a.entries, a.block_size
    e = fillseq_entries(n)
    out = {"workload": f"fillseq, {n} entries of 24 + 100 bytes, block_size {bs}", "entries": n}

    # ---- device-resident cut and emit ----
    d = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                          x.view(np.int32) if x.dtype == np.uint32 else x).cuda() for x in e]
    dk, dko, dkl, dv, dvo, dvl = d
    scr = torch.empty(int(L.lgs_block_build_scratch(n)), dtype=torch.uint8, device="cuda")
    first = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    roff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    rlen = torch.empty(n, dtype=torch.int32, device="cuda")
    ioff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")

    def cut():
        check(L.lgs_block_cut_dev(dk.data_ptr(), dko.data_ptr(), dkl.data_ptr(), dvl.data_ptr(), n,
                                  bs, 16, 1, first.data_ptr(), roff.data_ptr(), rlen.data_ptr(),
                                  ioff.data_ptr(), cnt.data_ptr(), scr.data_ptr(), scr.numel(),
                                  None), "lgs_block_cut_dev")

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

    t_cut = timed(cut)
    nb, raw_total, max_len, ikey_total = (int(x) for x in cnt.cpu())
    raw = torch.empty(raw_total + 16, dtype=torch.uint8, device="cuda")
    ikey = torch.empty(ikey_total + 16, dtype=torch.uint8, device="cuda")

    def emit():
        check(L.lgs_block_emit_dev(dk.data_ptr(), dko.data_ptr(), dkl.data_ptr(), dv.data_ptr(),
                                   dvo.data_ptr(), dvl.data_ptr(), n, 16, 1, nb, first.data_ptr(),
                                   roff.data_ptr(), rlen.data_ptr(), raw.data_ptr(),
                                   ioff.data_ptr(), ikey.data_ptr(), scr.data_ptr(), scr.numel(),
                                   None), "lgs_block_emit_dev")

    t_emit = timed(emit)
    moved = 124 * n + raw_total                  # entries read once, blocks written once
    half = (moved // 2 + 15) // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    t_copy = timed(lambda: check(L.lgs_hbm_copy_dev(dst.data_ptr(), src.data_ptr(), half, None),
                                 "lgs_hbm_copy_dev"))
    out.update({
        "blocks": nb, "raw_bytes": raw_total,
        "cut_ms": t_cut * 1e3, "emit_ms": t_emit * 1e3,
        "emit_bytes_moved": moved, "emit_GBps": moved / t_emit / 1e9,
        "hbm_copy_GBps_same_bytes": 2 * half / t_copy / 1e9,
        "emit_fraction_of_copy_rate": (moved / t_emit) / (2 * half / t_copy),
        "cut_scratch_bytes_per_entry": scr.numel() / n,
    })
    del d, dk, dko, dkl, dv, dvo, dvl, scr, raw, ikey, src, dst, first, roff, rlen, ioff
    torch.cuda.empty_cache()

    # ---- host arrays in, table file out ----
    t_first, img = host_build(L, check, e, n, bs)
    warm = []
    for _ in range(3):
        t, img = host_build(L, check, e, n, bs)
        warm.append(t)
    sha = hashlib.sha256(img).hexdigest()
    out.update({"table_build_host_first_s": t_first,
                "table_build_host_warm_s": float(np.median(warm)),
                "file_size": int(len(img)), "sha256": sha})

    # ---- the reference's block builder on one host core ----
    exe = os.path.join(ROOT, "oracle", "_ref", "lcdb", "build_table_batched.gpu")
    if not a.no_ref and os.path.exists(exe):
        tmp = tempfile.mkdtemp(prefix="lgs_tb_")
        try:
            r = subprocess.run([exe, os.path.join(tmp, "db"), str(n), str(bs)],
                               capture_output=True, text=True, timeout=900)
            ref = {k: float(v) for k, v in re.findall(r"(\w+_s)=([0-9.]+)", r.stdout)}
            ref["rc"] = r.returncode
            path = os.path.join(tmp, "db", "000001.ldb")
            if os.path.exists(path):
                with open(path, "rb") as f:
                    ref["sha256"] = hashlib.sha256(f.read()).hexdigest()
                ref["file_equal"] = ref["sha256"] == sha
            out["reference_build_table_batched"] = ref
            if ref.get("cut_s"):
                out["device_cut_emit_vs_reference_cut"] = ref["cut_s"] / (t_cut + t_emit)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    else:
        out["reference_build_table_batched"] = "not run"

    if a.c5:
        del img
        n5 = 32768000
        e5 = fillseq_entries(n5)
        t5, img5 = host_build(L, check, e5, n5, 4096)
        t5w, img5 = host_build(L, check, e5, n5, 4096)
        sha5 = hashlib.sha256(img5).hexdigest()
        with open(os.path.join(ROOT, "tests", "golden", "digests.json")) as f:
            want = json.load(f)["C5_table_2GiB"]
        out["c5"] = {"entries": n5, "table_build_host_first_s": t5,
                     "table_build_host_warm_s": t5w, "file_size": int(len(img5)),
                     "sha256": sha5, "sha256_equal": sha5 == want["sha256"]}

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))
    if out.get("c5", {}).get("sha256_equal") is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
