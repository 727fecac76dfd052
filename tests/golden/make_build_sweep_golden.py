#!/usr/bin/env python3
"""Generate tests/golden/build_sweep.bin from the REFERENCE table builder.

Run where make_split_golden.py runs: beside the reference checkout, after
oracle/lcdb.mk has compiled it; never on the GPU box.  Every case of
tests/build_sweep.py goes through tests/golden/split_driver.c (mode `split`):
lcdb's ldb_tablegen_* driven as ldb_do_compaction_work drives it
(db_impl.c:1399-1425) with the case's options and max_output_file_size.
Only each output file's entry count, size and SHA-256 are recorded.

Nothing recorded was computed by the code under test, and nothing is written
unless tools/sim_table_split.py (split_serial and split_blocks) reproduces
every file and the exact / + 1 pairs behave as build_sweep.py states.

Usage: python tests/golden/make_build_sweep_golden.py
"""
from __future__ import annotations

import hashlib
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import build_sweep as sweep  # noqa: E402
import sim_table_split as sim  # noqa: E402
from build_sweep_golden_io import PATH, Record, digest, write  # noqa: E402
from make_split_golden import compile_driver  # noqa: E402
from sim_block_cut import serial_blocks  # noqa: E402

MAX_FILES = 3000


def check_exact_pairs() -> None:
    for a, b, kind, at in sweep.exact_cases():
        es = sweep.entries(a.spec)
        if kind == "block":
            E, R = a.block_size, a.restart_interval
            f0, b0 = serial_blocks(es, E, R)
            f1, _ = serial_blocks(es, E + 1, R)
            assert 0 < at < len(b0) - 1 and len(b0[at]) == E, a.name
            assert f1[:at + 1] == f0[:at + 1] and f1[at + 1] > f0[at + 1], a.name
        else:
            M = a.max_file_size
            _, _, start, end = sweep.framed(es, a.block_size, a.restart_interval, a.compression)
            fb0, fb1 = sweep.file_blocks(start, end, M), sweep.file_blocks(start, end, M + 1)
            s, e = fb0[at]
            assert 0 < at < len(fb0) - 1 and end[e - 1] - start[s] == M, a.name
            assert fb1[:at] == fb0[:at] and fb1[at] == (s, e + 1), a.name
        print(f"  {a.name}: {kind} {at} exact at {E if kind == 'block' else M}")


def run_case(driver: str, tmp: str, idx: int, c) -> Record:
    es = sweep.entries(c.spec)
    r = Record(c.name, c.spec, *c.options(), count=len(es), digest=digest(es))
    od = os.path.join(tmp, "case%04d" % idx)
    os.makedirs(od)
    cp = os.path.join(od, "case")
    with open(cp, "wb") as f:
        f.write(struct.pack("<8I", c.block_size, c.restart_interval, c.compression, c.bits_per_key,
                            c.internal, c.max_file_size & 0xffffffff, c.max_file_size >> 32,
                            len(es)))
        pack = struct.Struct("<I").pack
        f.write(b"".join(pack(len(k)) + k + pack(len(v)) + v for k, v in es))
    subprocess.run([driver, "split", cp, od], check=True)
    rows = [[int(x) for x in ln.split()] for ln in open(os.path.join(od, "split.txt"))]
    images = [open(os.path.join(od, "%06d.ldb" % row[0]), "rb").read() for row in rows]
    for (_, n, size), img in zip(rows, images):
        assert size == len(img) and n > 0, c.name
        r.files.append((n, size, hashlib.sha256(img).digest()))
    assert sum(n for n, _, _ in r.files) == len(es), c.name
    t0 = time.process_time()
    first, mine = sim.split_serial(es, c.block_size, c.restart_interval, c.compression,
                                   c.bits_per_key, bool(c.internal), c.max_file_size)
    dt = time.process_time() - t0
    assert mine == images, f"{c.name}: the model's files differ from lcdb's"
    assert first == sim.split_blocks(es, c.block_size, c.restart_interval, c.compression,
                                     c.max_file_size), c.name
    print(f"  {c.name}: {len(es)} entries -> {len(images)} files (model {dt:.1f} s)")
    return r


def main() -> None:
    check_exact_pairs()
    cases = sweep.all_cases()
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        for i, c in enumerate(cases):
            records.append(run_case(driver, tmp, i, c))
            shutil.rmtree(os.path.join(tmp, "case%04d" % i))
    files = sum(len(r.files) for r in records)
    assert files <= MAX_FILES, files
    size = write(PATH, records)
    print(f"{PATH}: {len(records)} cases, {files} files, {size} bytes")
    assert size < 256 * 1024


if __name__ == "__main__":
    main()
