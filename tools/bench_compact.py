"""One compaction end to end on tools/bench_merge.py's workload:
1 048 576 fillseq entries (a 16-digit decimal user key + tag, 100-byte values)
dealt round-robin into k = 4 tables (lgs_table_build_host, default options:
4 KiB blocks, restart interval 16, Snappy, no filter), compacted with nothing
dropped and max_output_file_size = 2 MiB.

* compact_to_files end to end (open, scan, merge, build, download of the
  images), wall clock around a device synchronisation: median, minimum and
  maximum of --e2e-iters runs after one warm-up;
* compact_tables on the same inputs (one output file whatever its size), the
  same way.  The tool runs on a tree that has no compact_to_files as well and
  then measures only this: that is how the parent commit's figure is taken
  (--parent-json names its output, read for the ratio);
* the build alone, entries resident in the layout the merge leaves them in:
  lgs_tables_build_dev with 2 MiB files and with one file, by HIP events
  (median, minimum and maximum of --iters runs after two warm-ups), and from
  the two the time one more file costs (its tail: one synchronisation and a
  fixed number of launches);
* beside it lgs_hbm_copy_dev moving the framed data bytes once in and once
  out (the floor of the image assembly copy, whose own time comes from a
  separate run under `rocprofv3 --kernel-trace --stats`: pack_kernel);
* the result checked: the files' entry ranges cover the entries, the images
  of the timed build are the images compact_to_files returned, and the
  one-file image is what compact_tables returned (SHA-256, compared with the
  parent's when --parent-json is given).

--version measures the compaction inside a version instead:
compact_in_version on the same inputs against 64 level + 2 files of 1 MiB
spread over the key space, with a limit that lets about ten stops fire, and
compact_to_files beside it, both end to end as above; the result goes to
profiles/compact_version.json.

Writes one JSON object to --out (default profiles/compact.json) and prints it.
usage: python tools/bench_compact.py [--entries N] [--tables K] [--version]
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--entries", type=int, default=1 << 20)
    p.add_argument("--tables", type=int, default=4)
    p.add_argument("--max-file-size", type=int, default=2 << 20)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--e2e-iters", type=int, default=3)
    p.add_argument("--parent-json", default=None)
    p.add_argument("--build-only", action="store_true",
                   help="the build alone (for a kernel trace): no inputs, no end-to-end runs")
    p.add_argument("--version", action="store_true",
                   help="compact_in_version over --level-files level + 2 files, and "
                        "compact_to_files on the same inputs (DESIGN §4.10)")
    p.add_argument("--level-files", type=int, default=64)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles",
                             "compact_version.json" if a.version else "compact.json")

    import numpy as np
    import torch

    from bench_merge import deal_runs
    from bench_table_build import fillseq_entries
    from lcdb_amd import _native, table
    from lcdb_amd._native import check
    L = _native.lib()
    if L.lgs_device_count() <= 0:
        sys.exit("bench_compact: no GPU visible")
    torch.cuda.set_device(0)
    n, k = a.entries, a.tables
    e = fillseq_entries(n)
    out = {"workload": f"fillseq, {n} entries of 24 + 100 bytes dealt round-robin into {k} tables, "
                       f"default options, max_output_file_size {a.max_file_size}",
           "entries": n, "tables": k, "entry_bytes": 124 * n}

    def stats(ts):
        return {"median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3,
                "max_ms": max(ts) * 1e3}

    # The inputs: one table per run (the builder's host entry point on arrays).
    images = []
    for r in ([] if a.build_only else deal_runs(e, n, k)):
        m = r[6]
        cap = int(L.lgs_table_build_bound(m, 24 * m, 100 * m, 0))
        file = np.empty(cap, dtype=np.uint8)
        size = C.c_size_t(0)
        check(L.lgs_table_build_host(*(x.ctypes.data for x in r[:6]), m, 4096, 16, 1, 0, 1,
                                     file.ctypes.data, cap, C.byref(size)), "lgs_table_build_host")
        images.append(file[:size.value].copy())
    out["input_bytes"] = int(sum(len(i) for i in images))

    def wall(fn, iters):
        ts, res = [], None
        for i in range(iters + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if i >= 1:
                ts.append(time.perf_counter() - t0)
        return stats(ts), res

    if a.version:
        # The same inputs inside a version: level + 2 holds
        # --level-files files of 1 MiB over the key space with gaps between
        # them, and the limit lets about ten stops fire.  Nothing is dropped.
        nl = a.level_files
        span = n // nl
        tag = lambda s: ((s << 8) | 1).to_bytes(8, "little")      # noqa: E731
        lv = [(b"%016d" % (j * span + span // 8) + tag(5), b"%016d" % (j * span + span // 2) + tag(1),
               1 << 20) for j in range(nl)]
        limit = (nl << 20) // 10 - 1
        tv, fv = wall(lambda: table.compact_in_version(
            images, n + 1, [lv], max_output_file_size=a.max_file_size,
            max_grandparent_overlap_bytes=limit), a.e2e_iters)
        tp, fp = wall(lambda: table.compact_to_files(images, n + 1, False,
                                                     max_output_file_size=a.max_file_size),
                      a.e2e_iters)
        ok = sum(f["entries"] for f in fv) == n == sum(f["entries"] for f in fp)
        ok = ok and len(fv) > len(fp)
        # The same entries in the same order, cut in other places.
        out["workload"] += f"; level + 2: {nl} files of 1 MiB, limit {limit}"
        out["compact_in_version"] = dict(tv, files=len(fv), level_files=nl, limit=limit,
                                         output_bytes=sum(len(f["image"]) for f in fv))
        out["compact_to_files"] = dict(tp, files=len(fp),
                                       output_bytes=sum(len(f["image"]) for f in fp))
        out["in_version_vs_to_files"] = tv["median_ms"] / tp["median_ms"]
        out["ms_per_extra_file"] = (tv["median_ms"] - tp["median_ms"]) / (len(fv) - len(fp))
        out["verified"] = bool(ok)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(out, indent=1, sort_keys=True))
        if not ok:
            sys.exit("bench_compact: result check failed")
        return

    ok, one, files = True, None, None
    if not a.build_only:
        t, one = wall(lambda: table.compact_tables(images, n + 1, False), a.e2e_iters)
        out["compact_tables"] = dict(t, files=1, output_bytes=len(one),
                                     sha256=hashlib.sha256(one).hexdigest())
    if hasattr(table, "compact_to_files"):
        if not a.build_only:
            t, files = wall(lambda: table.compact_to_files(images, n + 1, False,
                                                           max_output_file_size=a.max_file_size),
                            a.e2e_iters)
            out["compact_to_files"] = dict(t, files=len(files),
                                           output_bytes=sum(len(f["image"]) for f in files))
            ok = ok and sum(f["entries"] for f in files) == n

        # The build alone: the merged entries as the merge leaves them.
        m = {kk: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else
                                  v.view(np.int32) if v.dtype == np.uint32 else v).cuda()
             for kk, v in zip(("keys", "key_off", "key_len", "vals", "val_off", "val_len"),
                              (e[0], np.arange(n + 1, dtype=np.uint64) * 24, e[2], e[3],
                               np.arange(n + 1, dtype=np.uint64) * 100, e[5]))}
        m.update(n=n, key_bytes=24 * n, val_bytes=100 * n)

        def timed(fn):
            ts, res = [], None
            for i in range(a.iters + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append(e0.elapsed_time(e1) / 1e3)
            return stats(ts), res

        t_split, b = timed(lambda: table.build_tables_dev(m, internal_keys=True,
                                                          max_file_size=a.max_file_size))
        t_one, b1 = timed(lambda: table.build_tables_dev(m, internal_keys=True))
        off, size = b["file_off"].cpu().numpy(), b["file_size"].cpu().numpy()
        host = b["files"].cpu().numpy()
        got = [host[int(o):int(o) + int(s)].tobytes() for o, s in zip(off, size)]
        nf = b["n_files"]
        ok = ok and (files is None or got == [f["image"] for f in files]) and b1["n_files"] == 1
        o1, s1 = int(b1["file_off"][0]), int(b1["file_size"][0])
        ok = ok and (one is None or b1["files"][o1:o1 + s1].cpu().numpy().tobytes() == one)
        first = b["file_first"].cpu().numpy()
        ok = ok and int(first[0]) == 0 and int(first[-1]) == n and bool((np.diff(first) > 0).all())
        out["build_split"] = dict(t_split, files=nf, ns_per_entry=t_split["median_ms"] * 1e6 / n,
                                  synchronisations=3 + nf + 1)
        out["build_one_file"] = dict(t_one, files=1, ns_per_entry=t_one["median_ms"] * 1e6 / n,
                                     synchronisations=3 + 1 + 1)
        if nf > 1:
            out["tail_ms_per_file"] = (t_split["median_ms"] - t_one["median_ms"]) / (nf - 1)
        data = int(sum(int(s) for s in size)) // 16 * 16
        src = torch.empty(data, dtype=torch.uint8, device="cuda")
        dst = torch.empty(data, dtype=torch.uint8, device="cuda")
        t_copy, _ = timed(lambda: check(L.lgs_hbm_copy_dev(dst.data_ptr(), src.data_ptr(), data,
                                                           None), "lgs_hbm_copy_dev"))
        out["hbm_copy_of_the_images"] = dict(t_copy, bytes=data,
                                             GBps=2 * data / (t_copy["median_ms"] / 1e3) / 1e9)
    if a.parent_json and os.path.exists(a.parent_json):
        par = json.load(open(a.parent_json))["compact_tables"]
        out["parent_compact_tables"] = par
        ok = ok and par["sha256"] == out["compact_tables"]["sha256"]
        out["compact_tables_vs_parent"] = par["median_ms"] / out["compact_tables"]["median_ms"]
        if "compact_to_files" in out:
            out["compact_to_files_vs_parent_compact_tables"] = \
                par["median_ms"] / out["compact_to_files"]["median_ms"]
            out["note"] = ("the parent's compact_tables writes one file whatever its size; "
                           "compact_to_files writes lcdb's files of max_output_file_size")
    out["verified"] = bool(ok)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    if not ok:
        sys.exit("bench_compact: result check failed")


if __name__ == "__main__":
    main()
