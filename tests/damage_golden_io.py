"""Reader for tests/golden/damage_get.bin and damage_scan.bin: what lcdb's own
ldb_table_open, ldb_table_internal_get and table iterator made of tables of
tests/golden/table_build.bin with seeded one-byte damage aimed at their
structures (tests/golden/make_damage_golden.py).

The two files have the layouts of table_get.bin and table_scan.bin
(table_get_golden_io.py, table_scan_golden_io.py) and hold the same cases in
the same order: a case's name is "<class>:<table>:<seed number>", its patches
are the damage, and a case whose table lcdb did not open has open_rc != 0 and
neither records nor runs.
"""
from __future__ import annotations

import os

import table_get_golden_io
import table_scan_golden_io

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GET_PATH = os.path.join(_GOLDEN, "damage_get.bin")
SCAN_PATH = os.path.join(_GOLDEN, "damage_scan.bin")
SIZE_CAP = 256 * 1024

CLASSES = ("entry_headers", "restart_arrays", "key_order", "index_block", "open_time", "framing")

# (tag, set name, (block size, restart interval, compression, bits per key))
TABLES = (
    ("fill256_c", "fill256", (256, 16, 1, 0)),
    ("fill256_r2", "fill256", (256, 2, 1, 10)),
    ("fill256i_r1", "fill256_internal", (256, 1, 0, 0)),
    ("fill4096i", "fill4096_internal", (4096, 16, 0, 0)),
    ("varint", "varint", (65536, 16, 0, 10)),
    ("varinti", "varint_internal", (65536, 16, 0, 10)),
    ("own_blocki", "own_block_internal", (1, 16, 0, 0)),
    ("bigvalue", "bigvalue", (4096, 16, 1, 0)),
)


def read_get() -> list:
    return table_get_golden_io.read(GET_PATH)


def read_scan() -> list:
    return table_scan_golden_io.read(SCAN_PATH)


def class_of(case) -> str:
    return case.name.split(":")[0]


def table_tag(case) -> str:
    return case.name.split(":")[1]
