"""SSTable block framing on the GPU.

lcdb stores every table block as ``contents | type | masked crc32c`` and
reads one back through ``ldb_read_block``.  This module is the Python face of
the batched C ABI that does both for many blocks per launch
(``include/lcdb_gpu_snappy.h``):

* ``crc32c_batch``    -- ``ldb_crc32c_value``/``extend``/``mask`` per block
  (src/util/crc32c.c:1147, crc32c.h:46-50);
* ``write_blocks``    -- ``ldb_tablegen_write_block`` for n data blocks
  (src/table/table_builder.c:123-213): encode, 12.5 % rule, trailer, packing;
* ``read_blocks``     -- ``ldb_read_block`` for n handles
  (src/table/format.c:162-270): truncation, checksum, type, raw or decode;
* ``*_host`` variants on host bytes (pinned staging inside the library);
* ``build_blocks``    -- ``ldb_tablegen_add``'s data blocks and index keys from
  sorted entries (src/table/table_builder.c:215-255, block_builder.c:91-158);
* ``build_table_host`` -- the whole ``.ldb`` of ``ldb_tablegen_*`` (:215-365);
* ``seek_blocks_host`` -- ``ldb_blockiter_seek`` for many (block, key) queries
  (src/table/block.c:324-451);
* ``get_host``        -- ``ldb_table_internal_get`` for many keys against one
  table image (src/table/table.c:314-364);
* ``open_table``      -- ``ldb_table_open`` once: the decoded index and filter
  blocks (and, if asked, the image) stay on the device, and ``.get`` /
  ``.get_dev`` are ``ldb_table_internal_get`` against them;
* ``block_entries`` / ``block_entries_host`` -- ``ldb_blockiter_first`` +
  ``_next`` until invalid for many decoded blocks (src/table/block.c:247-296,
  411-415): their entries in ``build_blocks``' input layout;
* ``OpenTable.scan`` / ``.scan_dev`` -- ``ldb_tableiter_create``, first or
  seek, next until invalid (src/table/two_level_iterator.c, table.c:229-311);
* ``merge_runs`` / ``merge_runs_host`` -- ``ldb_mergeiter_first`` + ``_next``
  until invalid over sorted runs (src/table/merger.c) and the drop loop of
  ``ldb_do_compaction_work`` (src/db_impl.c:1369-1396);
* ``build_tables_dev`` -- ``ldb_tablegen_*`` over entries in device memory, cut
  into the files of db_impl.c:1399-1425 by ``max_output_file_size``;
* ``compact_to_files`` / ``compact_tables`` -- scan, merge and drop, build:
  one compaction's output files (or one table) from its input tables;
* ``index_host``      -- ``ldb_table_open``'s footer, index-block handles and
  metaindex filter handle (src/table/table.c:78-180), the handles the batched
  read takes.

Everything runs through ``liblcdb_gpu_snappy.so``; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import _native
from ._native import (LGS_ENOSPC, LGS_GET_CORRUPT, LGS_GET_DELETED, LGS_GET_FOUND,
                      LGS_GET_NOTFOUND, LGS_NO_COMPRESSION, LGS_SNAPPY_COMPRESSION, LGS_ST_BADCRC,
                      LGS_ST_BADTYPE, LGS_ST_CORRUPT, LGS_ST_IOERR, LGS_ST_NOSPACE, LGS_ST_OK,
                      LGS_TRAILER_SIZE, check)
from .snappy import _stream_ptr

_L = _native.lib()

__all__ = [
    "crc32c_batch", "write_blocks", "read_blocks", "write_blocks_host", "read_blocks_host",
    "index_host", "FILTER_NAME", "seek_blocks_host", "block_entries", "block_entries_host", "ScanError", "merge_runs", "merge_runs_host", "merge_runs_version", "compact_tables", "compact_to_files", "compact_in_version", "build_tables_dev", "MergeError", "get_host", "open_table", "OpenTable", "build_blocks", "build_blocks_host", "build_table_host",
    "LGS_NO_COMPRESSION", "LGS_SNAPPY_COMPRESSION", "LGS_TRAILER_SIZE", "LGS_ST_OK",
    "LGS_ST_CORRUPT", "LGS_ST_NOSPACE", "LGS_ST_IOERR", "LGS_ST_BADCRC", "LGS_ST_BADTYPE",
    "LGS_GET_NOTFOUND", "LGS_GET_FOUND", "LGS_GET_DELETED", "LGS_GET_CORRUPT",
]


def _torch():
    import torch
    return torch


# ---------------------------------------------------------------------------
# Device-resident (torch tensors in HBM): offsets int64, lengths int32.
# ---------------------------------------------------------------------------

def crc32c_batch(d_in, d_off, d_len, d_type=None, masked: bool = True, d_crc=None, stream=None):
    """CRC32C of every block (followed by d_type[i] when given), masked by
    default: with a type this is each block's trailer crc field."""
    torch = _torch()
    n = int(d_len.numel())
    if d_crc is None:
        d_crc = torch.empty(n, dtype=torch.int32, device=d_in.device)
    check(_L.lgs_crc32c_batch_dev(d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                  d_type.data_ptr() if d_type is not None else None,
                                  1 if masked else 0, d_crc.data_ptr(), n, _stream_ptr(stream)),
          "lgs_crc32c_batch_dev")
    return d_crc


def write_buffers(n: int, raw_total: int, device, base: int = 0):
    """The output and scratch tensors of write_blocks, allocated once (a
    caller framing the same shape repeatedly passes them as `bufs`)."""
    torch = _torch()
    nscr = int(_L.lgs_table_write_scratch(n, raw_total))
    return (torch.empty(raw_total + LGS_TRAILER_SIZE * n + 16, dtype=torch.uint8, device=device),
            torch.empty(n, dtype=torch.int64, device=device),
            torch.empty(n, dtype=torch.int64, device=device),
            torch.full((1,), base, dtype=torch.int64, device=device),
            torch.empty(max(nscr, 1), dtype=torch.uint8, device=device))


def write_blocks(d_raw, d_off, d_len, compression: int = LGS_SNAPPY_COMPRESSION, base: int = 0,
                 max_len: Optional[int] = None, raw_total: Optional[int] = None, stream=None,
                 bufs=None):
    """Frame n raw data blocks into a contiguous file region.

    Returns (d_file, d_handle_off, d_handle_size, d_end): d_file[j] is file
    offset base + j, d_end[0] = base + bytes written (read it after the
    stream syncs).  d_raw must stay readable 16 bytes past every block.
    bufs: write_buffers(n, raw_total, device, base), reused."""
    torch = _torch()
    n = int(d_len.numel())
    dev = d_raw.device
    if max_len is None or raw_total is None:
        lens = d_len.to(torch.int64)
        max_len = int(lens.max()) if n else 0
        raw_total = int(lens.sum()) if n else 0
    d_file, hoff, hsize, end, scr = bufs if bufs is not None else write_buffers(n, raw_total, dev, base)
    nscr = int(scr.numel())
    check(_L.lgs_table_write_dev(d_raw.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                 int(max_len), int(raw_total), int(compression), int(base),
                                 d_file.data_ptr(), hoff.data_ptr(), hsize.data_ptr(),
                                 end.data_ptr(), scr.data_ptr(), nscr, _stream_ptr(stream)),
          "lgs_table_write_dev")
    return d_file, hoff, hsize, end


def read_blocks(d_file, file_len: int, d_hoff, d_hsize, d_out, d_out_off, d_out_cap,
                max_out_cap: int, verify: bool = True, d_out_len=None, d_status=None,
                stream=None, scratch=None):
    """ldb_read_block for every handle; returns (d_out_len, d_status).
    d_file must stay readable 16 bytes past file_len.  scratch: a uint8
    tensor of lgs_table_read_scratch(n) bytes, reused."""
    torch = _torch()
    n = int(d_hoff.numel())
    dev = d_file.device
    if d_out_len is None:
        d_out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    if d_status is None:
        d_status = torch.zeros(n, dtype=torch.uint8, device=dev)
    if scratch is None:
        scratch = torch.empty(max(int(_L.lgs_table_read_scratch(n)), 1), dtype=torch.uint8,
                              device=dev)
    scr = scratch
    nscr = int(scr.numel())
    check(_L.lgs_table_read_dev(d_file.data_ptr(), int(file_len), d_hoff.data_ptr(),
                                d_hsize.data_ptr(), n, 1 if verify else 0, d_out.data_ptr(),
                                d_out_off.data_ptr(), d_out_cap.data_ptr(), int(max_out_cap),
                                d_out_len.data_ptr(), d_status.data_ptr(), scr.data_ptr(), nscr,
                                _stream_ptr(stream)),
          "lgs_table_read_dev")
    return d_out_len, d_status


def build_blocks(d_keys, d_key_off, d_key_len, d_vals, d_val_off, d_val_len,
                 block_size: int = 4096, restart_interval: int = 16,
                 internal_keys: bool = False, stream=None):
    """lcdb's data blocks of n sorted entries (lgs_block_cut_dev + one
    read-back of the counts + lgs_block_emit_dev).

    Returns a dict of device tensors: ``raw`` (the packed blocks, 16 spare
    bytes), ``raw_off`` / ``raw_len`` (write_blocks' input), ``block_first``
    (nblocks + 1), ``ikey`` / ``ikey_off`` (nblocks + 1), and the ints
    ``nblocks``, ``raw_total``, ``max_len``.  Inputs must stay readable 16
    bytes past their end."""
    torch = _torch()
    n = int(d_key_len.numel())
    dev = d_keys.device
    sp = _stream_ptr(stream)
    scr = torch.empty(max(int(_L.lgs_block_build_scratch(n)), 1), dtype=torch.uint8, device=dev)
    first = torch.empty(n + 1, dtype=torch.int32, device=dev)
    raw_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    raw_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ikey_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    check(_L.lgs_block_cut_dev(d_keys.data_ptr(), d_key_off.data_ptr(), d_key_len.data_ptr(),
                               d_val_len.data_ptr(), n, int(block_size), int(restart_interval),
                               1 if internal_keys else 0, first.data_ptr(), raw_off.data_ptr(),
                               raw_len.data_ptr(), ikey_off.data_ptr(), counts.data_ptr(),
                               scr.data_ptr(), int(scr.numel()), sp), "lgs_block_cut_dev")
    if stream is not None:
        stream.synchronize()
    nb, raw_total, max_len, ikey_total = (int(x) for x in counts.cpu())
    raw = torch.empty(raw_total + 16, dtype=torch.uint8, device=dev)
    ikey = torch.empty(ikey_total + 16, dtype=torch.uint8, device=dev)
    check(_L.lgs_block_emit_dev(d_keys.data_ptr(), d_key_off.data_ptr(), d_key_len.data_ptr(),
                                d_vals.data_ptr(), d_val_off.data_ptr(), d_val_len.data_ptr(), n,
                                int(restart_interval), 1 if internal_keys else 0, nb,
                                first.data_ptr(), raw_off.data_ptr(), raw_len.data_ptr(),
                                raw.data_ptr(), ikey_off.data_ptr(), ikey.data_ptr(),
                                scr.data_ptr(), int(scr.numel()), sp), "lgs_block_emit_dev")
    if stream is not None:
        scr.record_stream(stream)
    return {"raw": raw, "raw_off": raw_off[:nb + 1], "raw_len": raw_len[:nb],
            "block_first": first[:nb + 1], "ikey": ikey, "ikey_off": ikey_off[:nb + 1],
            "nblocks": nb, "raw_total": raw_total, "max_len": max_len}


def block_entries(d_blocks, d_block_off, d_block_len, block_bytes: int, d_block_status=None,
                  d_walk_from=None, d_emit_from=None, internal_keys: bool = False, stream=None):
    """The entries of n decoded blocks, in walk order (lgs_block_entries_count_dev
    + one read-back of the counts + lgs_block_entries_emit_dev).

    d_blocks uint8, d_block_off int64, d_block_len int32, the optional
    d_block_status uint8 and d_walk_from / d_emit_from int32 (-1: not given);
    block_bytes: at least the sum of the lengths.  Returns a dict of device
    tensors ``keys``, ``vals`` (16 spare bytes each), ``key_off``, ``val_off``
    (int64, n + 1), ``key_len``, ``val_len`` (int32, n) -- build_blocks' input
    -- ``entry_first`` (int32, blocks + 1), ``status`` (uint8, blocks), and the
    ints ``n``, ``key_bytes``, ``val_bytes``, ``max_key``."""
    torch = _torch()
    nb = int(d_block_len.numel())
    dev = d_blocks.device
    sp = _stream_ptr(stream)
    scr = torch.empty(max(int(_L.lgs_block_entries_scratch(nb, int(block_bytes))), 1),
                      dtype=torch.uint8, device=dev)
    first = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
    status = torch.zeros(max(nb, 1), dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    head = (d_blocks.data_ptr(), d_block_off.data_ptr(), d_block_len.data_ptr(),
            ptr(d_block_status), nb, int(block_bytes), ptr(d_walk_from), ptr(d_emit_from),
            1 if internal_keys else 0)
    check(_L.lgs_block_entries_count_dev(*head, first.data_ptr(), status.data_ptr(),
                                         counts.data_ptr(), scr.data_ptr(), int(scr.numel()), sp),
          "lgs_block_entries_count_dev")
    if stream is not None:
        stream.synchronize()
    n, kb, vb, mk = (int(x) for x in counts.cpu())
    keys = torch.zeros(kb + 16, dtype=torch.uint8, device=dev)
    vals = torch.zeros(vb + 16, dtype=torch.uint8, device=dev)
    key_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    val_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    key_len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    val_len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    check(_L.lgs_block_entries_emit_dev(*head, n, keys.data_ptr(), key_off.data_ptr(),
                                        key_len.data_ptr(), vals.data_ptr(), val_off.data_ptr(),
                                        val_len.data_ptr(), scr.data_ptr(), int(scr.numel()), sp),
          "lgs_block_entries_emit_dev")
    if stream is not None:
        scr.record_stream(stream)
    return {"keys": keys, "key_off": key_off, "key_len": key_len[:n], "vals": vals,
            "val_off": val_off, "val_len": val_len[:n], "entry_first": first,
            "status": status[:nb], "n": n, "key_bytes": kb, "val_bytes": vb, "max_key": mk}


# ---------------------------------------------------------------------------
# Host bytes.
# ---------------------------------------------------------------------------

def _pack_entries(entries):
    """(keys, key_off, key_len, vals, val_off, val_len) numpy arrays."""
    n = len(entries)
    klen = np.array([len(k) for k, _ in entries], dtype=np.uint32)
    vlen = np.array([len(v) for _, v in entries], dtype=np.uint32)
    koff = np.zeros(n, dtype=np.uint64)
    voff = np.zeros(n, dtype=np.uint64)
    if n:
        koff[1:] = np.cumsum(klen[:-1], dtype=np.uint64)
        voff[1:] = np.cumsum(vlen[:-1], dtype=np.uint64)
    keys = np.frombuffer(b"".join(k for k, _ in entries) + b"\0" * 16, dtype=np.uint8)
    vals = np.frombuffer(b"".join(v for _, v in entries) + b"\0" * 16, dtype=np.uint8)
    return keys, koff, klen, vals, voff, vlen


def build_blocks_host(entries, block_size: int = 4096, restart_interval: int = 16,
                      internal_keys: bool = False):
    """Returns (data blocks, block_first, index keys) of sorted (key, value)
    entries: what ldb_tablegen_add cuts and adds to its index block."""
    import ctypes as C
    n = len(entries)
    keys, koff, klen, vals, voff, vlen = _pack_entries(entries)
    kb, vb = int(klen.sum()), int(vlen.sum())
    cap = int(_L.lgs_block_build_bound(n, kb, vb))
    raw = np.empty(cap, dtype=np.uint8)
    raw_off = np.zeros(n + 1, dtype=np.uint64)
    raw_len = np.zeros(max(n, 1), dtype=np.uint32)
    first = np.zeros(n + 1, dtype=np.uint32)
    ikey = np.empty(kb + 16, dtype=np.uint8)
    ikey_off = np.zeros(n + 1, dtype=np.uint64)
    nb = C.c_uint32(0)
    check(_L.lgs_block_build_host(keys.ctypes.data, koff.ctypes.data, klen.ctypes.data,
                                  vals.ctypes.data, voff.ctypes.data, vlen.ctypes.data, n,
                                  int(block_size), int(restart_interval),
                                  1 if internal_keys else 0, raw.ctypes.data, cap,
                                  raw_off.ctypes.data, raw_len.ctypes.data, first.ctypes.data,
                                  ikey.ctypes.data, kb + 16, ikey_off.ctypes.data, C.byref(nb)),
          "lgs_block_build_host")
    m = nb.value
    blocks = [raw[int(raw_off[b]):int(raw_off[b]) + int(raw_len[b])].tobytes() for b in range(m)]
    ikeys = [ikey[int(ikey_off[b]):int(ikey_off[b + 1])].tobytes() for b in range(m)]
    return blocks, [int(x) for x in first[:m + 1]], ikeys


def build_table_host(entries, block_size: int = 4096, restart_interval: int = 16,
                     compression: int = LGS_SNAPPY_COMPRESSION, bits_per_key: int = 0,
                     internal_keys: bool = False, file_cap: Optional[int] = None) -> bytes:
    """The .ldb lcdb's table builder writes for sorted (key, value) entries
    (lgs_table_build_host)."""
    import ctypes as C
    n = len(entries)
    keys, koff, klen, vals, voff, vlen = _pack_entries(entries)
    if file_cap is None:
        file_cap = int(_L.lgs_table_build_bound(n, int(klen.sum()), int(vlen.sum()),
                                                int(bits_per_key)))
    file = np.empty(max(int(file_cap), 1), dtype=np.uint8)
    size = C.c_size_t(0)
    check(_L.lgs_table_build_host(keys.ctypes.data, koff.ctypes.data, klen.ctypes.data,
                                  vals.ctypes.data, voff.ctypes.data, vlen.ctypes.data, n,
                                  int(block_size), int(restart_interval), int(compression),
                                  int(bits_per_key), 1 if internal_keys else 0,
                                  file.ctypes.data, int(file_cap), C.byref(size)),
          "lgs_table_build_host")
    return file[:size.value].tobytes()

def write_blocks_host(blocks: Sequence[bytes], compression: int = LGS_SNAPPY_COMPRESSION,
                      base: int = 0):
    """Returns (region bytes for file offsets [base, end), handle_off, handle_size, end)."""
    n = len(blocks)
    lens = np.array([len(b) for b in blocks], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    if n:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(blocks) + b"\0" * 16, dtype=np.uint8)
    cap = int(lens.sum()) + LGS_TRAILER_SIZE * n + 16
    file = np.empty(cap, dtype=np.uint8)
    hoff = np.zeros(n, dtype=np.uint64)
    hsize = np.zeros(n, dtype=np.uint64)
    end = np.zeros(1, dtype=np.uint64)
    check(_L.lgs_table_write_host(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, n,
                                  int(compression), int(base), file.ctypes.data, cap,
                                  hoff.ctypes.data, hsize.ctypes.data, end.ctypes.data),
          "lgs_table_write_host")
    e = int(end[0])
    return file[:e - base].tobytes(), hoff, hsize, e


def read_blocks_host(file, handle_off, handle_size, caps, verify: bool = True):
    """Returns (list of contents or None, status array) for every handle."""
    img = np.frombuffer(bytes(file), dtype=np.uint8) if not isinstance(file, np.ndarray) else file
    n = len(handle_off)
    hoff = np.ascontiguousarray(handle_off, dtype=np.uint64)
    hsize = np.ascontiguousarray(handle_size, dtype=np.uint64)
    cap = np.ascontiguousarray(caps, dtype=np.uint32)
    ooff = np.zeros(n, dtype=np.uint64)
    if n:
        ooff[1:] = np.cumsum(cap[:-1].astype(np.uint64))
    out = np.empty(int(cap.astype(np.uint64).sum()) + 16, dtype=np.uint8)
    olen = np.zeros(n, dtype=np.uint32)
    st = np.zeros(n, dtype=np.uint8)
    check(_L.lgs_table_read_host(img.ctypes.data if len(img) else None, len(img),
                                 hoff.ctypes.data, hsize.ctypes.data, n, 1 if verify else 0,
                                 out.ctypes.data, ooff.ctypes.data, cap.ctypes.data,
                                 olen.ctypes.data, st.ctypes.data),
          "lgs_table_read_host")
    res = [out[int(o):int(o) + int(k)].tobytes() if s == LGS_ST_OK else None
           for o, k, s in zip(ooff, olen, st)]
    return res, st


def _unpack_entries(keys, key_off, key_len, vals, val_off, val_len, n):
    kb, vb = keys.tobytes(), vals.tobytes()
    return [(kb[int(key_off[i]):int(key_off[i]) + int(key_len[i])],
             vb[int(val_off[i]):int(val_off[i]) + int(val_len[i])]) for i in range(n)]


def block_entries_host(blocks: Sequence[bytes], internal_keys: bool = False, block_status=None,
                       walk_from=None, emit_from=None, caps=None):
    """ldb_blockiter_first + _next until invalid for every decoded block
    (lgs_block_entries_host).  Returns ([[(key, value)] per block], status
    array).  walk_from / emit_from: per block an offset or None.  caps:
    (entries, key bytes, value bytes) to call with; by default one call with
    nothing sizes the outputs.  Too small raises ScanError with ``.needed``."""
    nb = len(blocks)
    blen = np.array([len(b) for b in blocks], dtype=np.uint32)
    boff = np.zeros(nb, dtype=np.uint64)
    if nb:
        boff[1:] = np.cumsum(blen[:-1], dtype=np.uint64)
    bbuf = np.frombuffer(b"".join(blocks) + b"\0" * 16, dtype=np.uint8)
    bst = None if block_status is None else np.ascontiguousarray(block_status, dtype=np.uint8)

    def offs(a):
        if a is None:
            return None
        return np.array([0xFFFFFFFF if x is None else x for x in a], dtype=np.uint32)

    wf, ef = offs(walk_from), offs(emit_from)
    first = np.zeros(nb + 1, dtype=np.uint32)
    status = np.zeros(max(nb, 1), dtype=np.uint8)
    needed = np.zeros(3, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data if a is not None else None   # noqa: E731

    def call(n, kb, vb):
        keys = np.zeros(kb + 16, dtype=np.uint8)
        vals = np.zeros(vb + 16, dtype=np.uint8)
        koff = np.zeros(n + 1, dtype=np.uint64)
        voff = np.zeros(n + 1, dtype=np.uint64)
        klen = np.zeros(max(n, 1), dtype=np.uint32)
        vlen = np.zeros(max(n, 1), dtype=np.uint32)
        rc = _L.lgs_block_entries_host(bbuf.ctypes.data, boff.ctypes.data, blen.ctypes.data,
                                       ptr(bst), nb, ptr(wf), ptr(ef), 1 if internal_keys else 0,
                                       first.ctypes.data, status.ctypes.data, keys.ctypes.data, kb,
                                       koff.ctypes.data, klen.ctypes.data, vals.ctypes.data, vb,
                                       voff.ctypes.data, vlen.ctypes.data, n, needed.ctypes.data)
        return rc, (keys, koff, klen, vals, voff, vlen)

    rc, out = call(*(caps if caps is not None else (0, 0, 0)))
    if rc == LGS_ENOSPC and caps is None:
        rc, out = call(*(int(x) for x in needed))
    if rc == LGS_ENOSPC:
        e = ScanError("lgs_block_entries_host: outputs too small")
        e.needed = tuple(int(x) for x in needed)
        e.untouched = not (out[0].any() or out[3].any() or out[2].any() or out[5].any())
        raise e
    check(rc, "lgs_block_entries_host")
    flat = _unpack_entries(*out, int(needed[0]))
    return [flat[int(first[b]):int(first[b + 1])] for b in range(nb)], status[:nb]


FILTER_NAME = "filter.leveldb.BuiltinBloomFilter2"   # "filter." + bloom.c's policy name


def index_host(file, paranoid_checks: bool = False, internal_keys: bool = False,
               filter_name: str | None = FILTER_NAME, cap: int | None = None):
    """ldb_table_open's view of a table file (lgs_table_index_host): returns
    (handles [(offset, size)], separator keys, filter handle or None, status)."""
    import ctypes as C
    raw = bytes(file)
    img = np.frombuffer(raw + b"\0", dtype=np.uint8)
    cap = cap if cap is not None else max(1, len(raw) // 8)
    hoff = np.zeros(cap, dtype=np.uint64)
    hsize = np.zeros(cap, dtype=np.uint64)
    keys = np.zeros(max(1, len(raw)), dtype=np.uint8)
    koff = np.zeros(cap + 1, dtype=np.uint64)
    count = C.c_uint32(0)
    foff, fsize = C.c_uint64(0), C.c_uint64(0)
    st = C.c_uint8(0)
    check(_L.lgs_table_index_host(img.ctypes.data, len(raw), int(paranoid_checks),
                                  int(internal_keys),
                                  filter_name.encode() if filter_name else None,
                                  hoff.ctypes.data, hsize.ctypes.data, cap, C.byref(count),
                                  keys.ctypes.data, len(keys), koff.ctypes.data, C.byref(foff),
                                  C.byref(fsize), C.byref(st)),
          "lgs_table_index_host")
    n = count.value
    handles = [(int(hoff[i]), int(hsize[i])) for i in range(n)]
    ks = [keys[int(koff[i]):int(koff[i + 1])].tobytes() for i in range(n)]
    fh = None if foff.value == (1 << 64) - 1 else (foff.value, fsize.value)
    return handles, ks, fh, st.value


def _pack_keys(keys):
    """(bytes + 16 spare, key_off u64, key_len u32) numpy arrays."""
    n = len(keys)
    klen = np.array([len(k) for k in keys], dtype=np.uint32)
    koff = np.zeros(n, dtype=np.uint64)
    if n:
        koff[1:] = np.cumsum(klen[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(keys) + b"\0" * 16, dtype=np.uint8)
    return buf, koff, klen


def seek_blocks_host(blocks: Sequence[bytes], queries, internal_keys: bool = False,
                     block_status=None):
    """ldb_blockiter_create + ldb_blockiter_seek for every query (block index,
    key) against the decoded `blocks` (lgs_block_seek_dev on uploaded copies).

    Returns ([(entry_pos, key, value) or None], status array)."""
    torch = _torch()
    nb, nq = len(blocks), len(queries)
    if nq == 0:
        return [], np.zeros(0, dtype=np.uint8)
    dev = torch.device("cuda")
    blen = np.array([len(b) for b in blocks], dtype=np.uint32)
    boff = np.zeros(nb, dtype=np.uint64)
    if nb:
        boff[1:] = np.cumsum(blen[:-1], dtype=np.uint64)
    bbuf = np.frombuffer(b"".join(blocks) + b"\0" * 16, dtype=np.uint8)
    kbuf, koff, klen = _pack_keys([k for _, k in queries])
    qb = np.array([b for b, _ in queries], dtype=np.uint32)

    def up(a, dt):
        return torch.from_numpy(a.view(dt).copy()).to(dev)

    d_b, d_boff, d_blen = up(bbuf, np.uint8), up(boff, np.int64), up(blen, np.int32)
    d_k, d_koff, d_klen = up(kbuf, np.uint8), up(koff, np.int64), up(klen, np.int32)
    d_qb = up(qb, np.int32)
    d_bst = None if block_status is None else up(np.asarray(block_status, dtype=np.uint8), np.uint8)
    i32 = lambda: torch.empty(nq, dtype=torch.int32, device=dev)   # noqa: E731
    d_pos, d_fkl, d_vpos, d_vlen = i32(), i32(), i32(), i32()
    d_st = torch.empty(nq, dtype=torch.uint8, device=dev)
    scr = torch.empty(max(int(_L.lgs_block_seek_scratch(nq)), 1), dtype=torch.uint8, device=dev)

    def run(d_kout, d_kout_off, d_kout_cap):
        check(_L.lgs_block_seek_dev(
            d_b.data_ptr(), d_boff.data_ptr(), d_blen.data_ptr(),
            d_bst.data_ptr() if d_bst is not None else None, nb, d_qb.data_ptr(), d_k.data_ptr(),
            d_koff.data_ptr(), d_klen.data_ptr(), nq, 1 if internal_keys else 0, d_pos.data_ptr(),
            d_fkl.data_ptr(), d_vpos.data_ptr(), d_vlen.data_ptr(), d_st.data_ptr(),
            d_kout.data_ptr() if d_kout is not None else None,
            d_kout_off.data_ptr() if d_kout is not None else None,
            d_kout_cap.data_ptr() if d_kout is not None else None,
            scr.data_ptr(), int(scr.numel()), None), "lgs_block_seek_dev")
        torch.cuda.synchronize()

    run(None, None, None)                     # the lengths, then the keys
    fkl = d_fkl.cpu().numpy().view(np.uint32)
    cap = fkl.copy()
    ooff = np.zeros(nq, dtype=np.uint64)
    ooff[1:] = np.cumsum(cap[:-1], dtype=np.uint64)
    d_kout = torch.zeros(int(cap.astype(np.uint64).sum()) + 16, dtype=torch.uint8, device=dev)
    run(d_kout, up(ooff, np.int64), up(cap, np.int32))
    pos = d_pos.cpu().numpy().view(np.uint32)
    vpos = d_vpos.cpu().numpy().view(np.uint32)
    vlen = d_vlen.cpu().numpy().view(np.uint32)
    st = d_st.cpu().numpy()
    kout = d_kout.cpu().numpy()
    res = []
    for q in range(nq):
        if pos[q] == 0xFFFFFFFF:
            res.append(None)
            continue
        blk = blocks[int(qb[q])]
        res.append((int(pos[q]), kout[int(ooff[q]):int(ooff[q]) + int(fkl[q])].tobytes(),
                    blk[int(vpos[q]):int(vpos[q]) + int(vlen[q])]))
    return res, st


def get_host(file, keys: Sequence[bytes], verify: bool = True, paranoid_checks: bool = False,
             internal_keys: bool = False, filter_name: str | None = FILTER_NAME,
             out_cap: Optional[int] = None):
    """ldb_table_internal_get for every key against one table image
    (lgs_table_get_host).  Returns ([(key, value) or None], status, verdict)."""
    import ctypes as C
    raw = bytes(file)
    img = np.frombuffer(raw + b"\0", dtype=np.uint8)
    nq = len(keys)
    kbuf, koff, klen = _pack_keys(list(keys))
    called = np.zeros(max(nq, 1), dtype=np.uint8)
    status = np.zeros(max(nq, 1), dtype=np.uint8)
    verdict = np.zeros(max(nq, 1), dtype=np.uint8)
    okoff = np.zeros(nq + 1, dtype=np.uint64)
    ovoff = np.zeros(nq + 1, dtype=np.uint64)
    need = C.c_size_t(0)
    cap = int(out_cap) if out_cap is not None else max(4096, 128 * nq)
    for attempt in range(2):
        out = np.empty(max(cap, 1), dtype=np.uint8)
        rc = _L.lgs_table_get_host(img.ctypes.data, len(raw), 1 if verify else 0,
                                   1 if paranoid_checks else 0, 1 if internal_keys else 0,
                                   filter_name.encode() if filter_name else None,
                                   kbuf.ctypes.data, koff.ctypes.data, klen.ctypes.data, nq,
                                   called.ctypes.data, status.ctypes.data, verdict.ctypes.data,
                                   out.ctypes.data, cap, okoff.ctypes.data, ovoff.ctypes.data,
                                   C.byref(need))
        if rc != LGS_ENOSPC or attempt:
            break
        cap = need.value                       # one retry with the size it asked for
    check(rc, "lgs_table_get_host")
    res = []
    for q in range(nq):
        if not called[q]:
            res.append(None)
            continue
        a, b, c = int(okoff[q]), int(ovoff[q]), int(okoff[q + 1])
        res.append((out[a:b].tobytes(), out[b:c].tobytes()))
    return res, status[:nq], verdict[:nq]


class ScanError(_native.LgsError):
    """A scan that ended in a status other than LGS_ST_OK (``.status``), or
    outputs too small for lgs_block_entries_host (``.needed``)."""


class OpenTable:
    """A table opened once (lgs_table_open_host): the decoded index and filter
    blocks stay on the device, and every ``get`` runs against them.  With
    ``resident`` the whole image does, and ``get_dev`` serves keys and results
    in device memory.  Also a context manager; ``close`` is idempotent."""

    def __init__(self, file, paranoid_checks: bool = False, internal_keys: bool = False,
                 filter_name: str | None = FILTER_NAME, resident: bool = False):
        import ctypes as C
        # A borrowed image must outlive the handle: a numpy array is kept as it
        # is (the caller's buffer), anything else is copied once.
        if isinstance(file, np.ndarray) and file.dtype == np.uint8 and file.flags.c_contiguous:
            img = file
        else:
            img = np.frombuffer(bytes(file), dtype=np.uint8)
        self._len = len(img)
        self._img = img if len(img) else np.zeros(1, dtype=np.uint8)
        self.internal_keys = bool(internal_keys)
        self.resident = bool(resident)
        h, st = C.c_void_p(None), C.c_uint8(0)
        check(_L.lgs_table_open_host(self._img.ctypes.data, self._len,
                                     1 if paranoid_checks else 0, 1 if internal_keys else 0,
                                     filter_name.encode() if filter_name else None,
                                     1 if resident else 0, C.byref(h), C.byref(st)),
              "lgs_table_open_host")
        self._h = h
        self.status = st.value
        if resident:
            self._img = None                  # the call has uploaded it

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            _L.lgs_table_close(h)
        self._img = None

    def _handle(self):
        if self._h is None:
            raise ValueError("the table is closed")
        return self._h

    def info(self) -> dict:
        """lgs_table_info: status, resident, index_bytes, filter_bytes, device_bytes."""
        import ctypes as C
        st, res = C.c_uint8(0), C.c_int(0)
        ib, fb, db = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(_L.lgs_table_info(self._handle(), C.byref(st), C.byref(res), C.byref(ib),
                                C.byref(fb), C.byref(db)), "lgs_table_info")
        return {"status": st.value, "resident": bool(res.value), "index_bytes": ib.value,
                "filter_bytes": fb.value, "device_bytes": db.value}

    def get(self, keys: Sequence[bytes], verify: bool = True, out_cap: Optional[int] = None):
        """ldb_table_internal_get for every key (lgs_table_get): what get_host
        returns, ([(key, value) or None], status, verdict)."""
        import ctypes as C
        nq = len(keys)
        kbuf, koff, klen = _pack_keys(list(keys))
        called = np.zeros(max(nq, 1), dtype=np.uint8)
        status = np.zeros(max(nq, 1), dtype=np.uint8)
        verdict = np.zeros(max(nq, 1), dtype=np.uint8)
        okoff = np.zeros(nq + 1, dtype=np.uint64)
        ovoff = np.zeros(nq + 1, dtype=np.uint64)
        need = C.c_size_t(0)
        cap = int(out_cap) if out_cap is not None else max(4096, 128 * nq)
        for attempt in range(2):
            out = np.empty(max(cap, 1), dtype=np.uint8)
            rc = _L.lgs_table_get(self._handle(), 1 if verify else 0, kbuf.ctypes.data,
                                  koff.ctypes.data, klen.ctypes.data, nq, called.ctypes.data,
                                  status.ctypes.data, verdict.ctypes.data, out.ctypes.data, cap,
                                  okoff.ctypes.data, ovoff.ctypes.data, C.byref(need))
            if rc != LGS_ENOSPC or attempt:
                break
            cap = need.value                   # one retry with the size it asked for
        check(rc, "lgs_table_get")
        res = []
        for q in range(nq):
            if not called[q]:
                res.append(None)
                continue
            a, b, c = int(okoff[q]), int(ovoff[q]), int(okoff[q + 1])
            res.append((out[a:b].tobytes(), out[b:c].tobytes()))
        return res, status[:nq], verdict[:nq]

    def get_dev(self, d_keys, d_key_off, d_key_len, verify: bool = True,
                out_cap: Optional[int] = None, stream=None):
        """lgs_table_get_dev on torch device tensors (uint8 keys readable 16
        bytes past their end, int64 offsets, int32 lengths; resident tables
        only).  Returns a dict of device tensors ``called``, ``status``,
        ``verdict`` (uint8, nq), ``out`` (uint8), ``out_key_off`` and
        ``out_val_off`` (int64, nq + 1), and the int ``out_needed``; complete
        on the stream when it returns.  One retry on LGS_ENOSPC, as ``get``."""
        import ctypes as C
        torch = _torch()
        nq = int(d_key_len.numel())
        dev = d_keys.device
        u8 = lambda n: torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)   # noqa: E731
        called, status, verdict = u8(nq), u8(nq), u8(nq)
        okoff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        ovoff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        need = C.c_size_t(0)
        cap = int(out_cap) if out_cap is not None else max(4096, 128 * nq)
        sp = _stream_ptr(stream)
        for attempt in range(2):
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            rc = _L.lgs_table_get_dev(self._handle(), 1 if verify else 0, d_keys.data_ptr(),
                                      d_key_off.data_ptr(), d_key_len.data_ptr(), nq,
                                      called.data_ptr(), status.data_ptr(), verdict.data_ptr(),
                                      out.data_ptr(), cap, okoff.data_ptr(), ovoff.data_ptr(),
                                      C.byref(need), sp)
            if rc != LGS_ENOSPC or attempt:
                break
            cap = need.value
        check(rc, "lgs_table_get_dev")
        return {"called": called[:nq], "status": status[:nq], "verdict": verdict[:nq], "out": out,
                "out_key_off": okoff, "out_val_off": ovoff, "out_needed": need.value}

    # ---- forward scans (lgs_table_scan, lgs_table_scan_dev) ----

    def _scan_call(self, fn, dev, verify, start, first_block, max_blocks, caps, stream=None):
        """One window: (dict, raw arrays) with the capacities grown as the
        call asks (LGS_ENOSPC reports the sizes; at most three calls)."""
        import ctypes as C
        torch = _torch() if dev is not None else None
        n_cap, k_cap, v_cap = caps
        sk = np.frombuffer((start or b"") + b"\0" * 16, dtype=np.uint8)
        done, nxt, at_end = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
        ist = C.c_uint8(0)
        needed = np.zeros(4, dtype=np.uint64)
        for _ in range(4):
            if dev is None:
                mk = lambda n, dt: np.zeros(max(n, 1), dtype=dt)   # noqa: E731
                ptr = lambda a: a.ctypes.data   # noqa: E731
                t8, t32, t64 = np.uint8, np.uint32, np.uint64
            else:
                mk = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)   # noqa: E731
                ptr = lambda a: a.data_ptr()   # noqa: E731
                t8, t32, t64 = torch.uint8, torch.int32, torch.int64
            keys, vals = mk(k_cap, t8), mk(v_cap, t8)
            koff, voff = mk(n_cap + 1, t64), mk(n_cap + 1, t64)
            klen, vlen = mk(n_cap, t32), mk(n_cap, t32)
            first, bst = mk(max_blocks + 1, t32), mk(max_blocks, t8)
            args = [self._handle(), 1 if verify else 0, sk.ctypes.data, len(start or b""),
                    1 if start is not None else 0, int(first_block), int(max_blocks), ptr(keys),
                    k_cap, ptr(koff), ptr(klen), ptr(vals), v_cap, ptr(voff), ptr(vlen), n_cap,
                    ptr(first), ptr(bst), C.byref(done), C.byref(nxt), C.byref(at_end),
                    C.byref(ist), needed.ctypes.data]
            if dev is not None:
                args.append(_stream_ptr(stream))
            rc = fn(*args)
            if rc != LGS_ENOSPC:
                break
            grow = lambda cap, need: cap if cap >= need else need + need // 8   # noqa: E731
            n_cap = grow(n_cap, int(needed[0]))
            k_cap = grow(k_cap, int(needed[1]))
            v_cap = grow(v_cap, int(needed[2]))
            max_blocks = max(max_blocks, int(needed[3]))
        check(rc, "lgs_table_scan_dev" if dev is not None else "lgs_table_scan")
        nb, n = done.value, int(needed[0])
        return {"keys": keys, "key_off": koff[:n + 1], "key_len": klen[:n], "vals": vals,
                "val_off": voff[:n + 1], "val_len": vlen[:n], "block_entry_first": first[:nb + 1],
                "block_status": bst[:nb], "n": n, "key_bytes": int(needed[1]),
                "val_bytes": int(needed[2]), "blocks_done": nb, "next_block": nxt.value,
                "at_end": bool(at_end.value), "index_status": ist.value,
                "caps": (n_cap, k_cap, v_cap)}

    def scan_window(self, start: Optional[bytes] = None, first_block: int = 0,
                    max_blocks: int = 1024, verify: bool = True, caps=(0, 0, 0)):
        """One call of lgs_table_scan: the entries of index entries
        [first_block, first_block + max_blocks) (with ``start``: from the
        block its seek names).  Returns a dict: ``entries`` [(key, value)],
        ``block_entry_first``, ``block_status``, ``blocks_done``,
        ``next_block``, ``at_end``, ``index_status``, ``caps``."""
        r = self._scan_call(_L.lgs_table_scan, None, verify, start, first_block, max_blocks, caps)
        r["entries"] = _unpack_entries(r["keys"], r["key_off"], r["key_len"], r["vals"],
                                       r["val_off"], r["val_len"], r["n"])
        return r

    def scan(self, start: Optional[bytes] = None, end: Optional[bytes] = None,
             verify: bool = True, max_blocks: int = 1024):
        """ldb_tableiter_create, first (or seek(start)), next until invalid: a
        generator of (key, value), a window of ``max_blocks`` index entries a
        call.  Stops before the first key with compare(key, end) >= 0 under
        the table's comparator, in order across windows (a caller's ``while
        valid && cmp(key, end) < 0``).  ``self.scan_status`` is the
        iterator's status where the generator stopped; a status other than
        LGS_ST_OK at the end raises ScanError after the last entry."""
        import struct

        def before_end(k: bytes) -> bool:
            if end is None:
                return True
            if not self.internal_keys:
                return k < end
            if k[:-8] != end[:-8]:
                return k[:-8] < end[:-8]
            return struct.unpack("<Q", k[-8:])[0] > struct.unpack("<Q", end[-8:])[0]

        self.scan_status = LGS_ST_OK
        saved, nxt, first, caps = LGS_ST_OK, 0, True, (0, 0, 0)
        while True:
            r = self.scan_window(start if first else None, nxt, max_blocks, verify, caps)
            first, caps, ef = False, r["caps"], r["block_entry_first"]
            for j in range(r["blocks_done"]):
                for k, v in r["entries"][int(ef[j]):int(ef[j + 1])]:
                    if not before_end(k):
                        self.scan_status = saved
                        return
                    yield k, v
                if saved == LGS_ST_OK and int(r["block_status"][j]) != LGS_ST_OK:
                    saved = int(r["block_status"][j])     # ldb_twoiter_saverr keeps the first
            nxt = r["next_block"]
            if r["at_end"]:
                break
        self.scan_status = r["index_status"] if r["index_status"] != LGS_ST_OK else saved
        if self.scan_status != LGS_ST_OK:
            e = ScanError(f"table scan ended with status {self.scan_status}")
            e.status = self.scan_status
            raise e

    def scan_dev(self, start: Optional[bytes] = None, first_block: int = 0,
                 max_blocks: int = 1024, verify: bool = True, caps=(0, 16, 16), stream=None,
                 device=None):
        """lgs_table_scan_dev: one window with every array a device tensor
        (resident tables only).  ``keys`` / ``key_off`` (int64, n + 1) /
        ``key_len`` (int32, n) / ``vals`` / ``val_off`` / ``val_len`` are
        build_blocks' input as they stand (16 spare bytes); also
        ``block_entry_first``, ``block_status`` and the host values
        ``n``, ``blocks_done``, ``next_block``, ``at_end``, ``index_status``.
        Complete on the stream when it returns."""
        torch = _torch()
        dev = torch.device("cuda") if device is None else device
        return self._scan_call(_L.lgs_table_scan_dev, dev, verify, start, first_block, max_blocks,
                               caps, stream)


def open_table(file, paranoid_checks: bool = False, internal_keys: bool = False,
               filter_name: str | None = FILTER_NAME, resident: bool = False) -> OpenTable:
    """ldb_table_open once (lgs_table_open_host).  With ``resident=False`` the
    image is borrowed: pass a numpy uint8 array and keep it unchanged in its
    data blocks while the table is open (bytes are copied once instead)."""
    return OpenTable(file, paranoid_checks, internal_keys, filter_name, resident)


# ---------------------------------------------------------------------------
# Merging sorted runs (lgs_merge_*).
# ---------------------------------------------------------------------------

class MergeError(_native.LgsError):
    """A merge the library refused: ``.rc`` (LGS_EINVAL for a run that is not
    sorted or holds a short internal key, then ``.run`` names it where known;
    LGS_ENOSPC for outputs too small, then ``.needed`` and ``.untouched``)."""


_NO_RUN = (1 << 64) - 1


def merge_runs(runs, internal_keys: bool = False, drop: bool = False, smallest_snapshot: int = 0,
               drop_deletions: bool = False, stream=None):
    """ldb_mergeiter_first + _next until invalid over sorted runs in device
    memory, then (``drop``, internal keys only) compaction's drop rule
    (lgs_merge_plan_dev + one read-back of the counts + lgs_merge_emit_dev).

    A run is a dict as ``block_entries`` / ``OpenTable.scan_dev`` return it:
    ``keys``, ``key_off``, ``key_len``, ``vals``, ``val_off``, ``val_len`` and
    optionally ``n``.  Among equal keys the lowest-numbered run comes first.
    Returns the same dict shape (``build_blocks``' input as it stands) plus
    ``src_run`` / ``src_index`` (int32, per kept entry) and the ints ``n``,
    ``dropped``, ``key_bytes``, ``val_bytes``, ``max_key``.  Raises MergeError
    for a run that is not sorted.  The runs must stay alive until the stream
    has passed the call."""
    torch = _torch()
    k = len(runs)
    arr = (_native.LgsRun * max(k, 1))()
    n_total = 0
    dev = None
    for r, run in enumerate(runs):
        n = int(run["n"]) if "n" in run else int(run["key_len"].numel())
        dev = run["keys"].device if dev is None else dev
        arr[r] = _native.LgsRun(*(run[f].data_ptr() for f in
                                  ("keys", "key_off", "key_len", "vals", "val_off", "val_len")), n)
        n_total += n
    dev = torch.device("cuda") if dev is None else dev
    sp = _stream_ptr(stream)
    scr = torch.empty(max(int(_L.lgs_merge_scratch(min(n_total, 0x7fffffff),
                                                   min(k, _native.LGS_MERGE_MAX_RUNS))), 1),
                      dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    check(_L.lgs_merge_plan_dev(arr, k, 1 if internal_keys else 0, 1 if drop else 0,
                                int(smallest_snapshot), 1 if drop_deletions else 0,
                                counts.data_ptr(), scr.data_ptr(), int(scr.numel()), sp),
          "lgs_merge_plan_dev")
    if stream is not None:
        stream.synchronize()
    cnt = [int(x) & _NO_RUN for x in counts.cpu()]
    if cnt[5] != _NO_RUN:
        e = MergeError(f"lgs_merge_plan_dev: run {cnt[5]} is not sorted or has a short key")
        e.rc, e.run = _native.LGS_EINVAL, cnt[5]
        raise e
    n, kb, vb, mk, dropped = cnt[:5]
    keys = torch.empty(kb + 16, dtype=torch.uint8, device=dev)
    vals = torch.empty(vb + 16, dtype=torch.uint8, device=dev)
    key_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    val_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    i32 = lambda: torch.empty(max(n, 1), dtype=torch.int32, device=dev)   # noqa: E731
    key_len, val_len, src_run, src_index = i32(), i32(), i32(), i32()
    check(_L.lgs_merge_emit_dev(arr, k, n, keys.data_ptr(), key_off.data_ptr(),
                                key_len.data_ptr(), vals.data_ptr(), val_off.data_ptr(),
                                val_len.data_ptr(), src_run.data_ptr(), src_index.data_ptr(),
                                scr.data_ptr(), int(scr.numel()), sp), "lgs_merge_emit_dev")
    if stream is not None:
        scr.record_stream(stream)
    return {"keys": keys, "key_off": key_off, "key_len": key_len[:n], "vals": vals,
            "val_off": val_off, "val_len": val_len[:n], "src_run": src_run[:n],
            "src_index": src_index[:n], "n": n, "dropped": dropped, "key_bytes": kb,
            "val_bytes": vb, "max_key": mk}


def _pack_levels(levels):
    """levels ([[(smallest, largest, file_size)]]) as an lgs_level array; the
    second value keeps the memory it points into alive."""
    import ctypes as C
    arr = (_native.LgsLevel * max(len(levels), 1))()
    keep, nfiles, key_bytes = [], 0, 0
    for v, files in enumerate(levels):
        fa = (_native.LgsLevelFile * max(len(files), 1))()
        for f, (lo, hi, size) in enumerate(files):
            lo, hi = bytes(lo), bytes(hi)
            bl, bh = C.create_string_buffer(lo, len(lo) + 1), C.create_string_buffer(hi, len(hi) + 1)
            keep += [bl, bh]
            fa[f] = _native.LgsLevelFile(C.addressof(bl), len(lo), C.addressof(bh), len(hi), int(size))
            key_bytes += len(lo) + len(hi)
        keep.append(fa)
        arr[v] = _native.LgsLevel(fa, len(files))
        nfiles += len(files)
    return arr, keep, nfiles, key_bytes


def merge_runs_version(runs, smallest_snapshot: int, levels, max_grandparent_overlap_bytes: int,
                       stream=None):
    """``merge_runs`` with internal keys and the drop rule for a compaction
    inside a version (lgs_merge_plan_version_dev + lgs_merge_emit_dev +
    lgs_merge_stops_dev).

    ``levels``: the files of the levels below the output, level + 2 first, at
    most 5 lists of ``(smallest_ikey, largest_ikey, file_size)`` in each
    level's order.  A deletion at or under ``smallest_snapshot`` is dropped
    where ldb_compaction_is_base_level_for_key holds for its user key, and
    ldb_compaction_should_stop_before runs against ``levels[0]`` with the
    limit ``max_grandparent_overlap_bytes``.  Returns ``merge_runs``' dict
    plus ``forced`` (int32 per kept entry: 1 where a stop closed the open
    output file just before it) and the int ``n_forced``."""
    torch = _torch()
    k = len(runs)
    arr = (_native.LgsRun * max(k, 1))()
    n_total = 0
    dev = None
    for r, run in enumerate(runs):
        n = int(run["n"]) if "n" in run else int(run["key_len"].numel())
        dev = run["keys"].device if dev is None else dev
        arr[r] = _native.LgsRun(*(run[f].data_ptr() for f in
                                  ("keys", "key_off", "key_len", "vals", "val_off", "val_len")), n)
        n_total += n
    dev = torch.device("cuda") if dev is None else dev
    sp = _stream_ptr(stream)
    lv, alive, nfiles, key_bytes = _pack_levels(levels)
    scr = torch.empty(max(int(_L.lgs_merge_version_scratch(
        min(n_total, 0x7fffffff), min(k, _native.LGS_MERGE_MAX_RUNS), nfiles, key_bytes)), 1),
        dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    check(_L.lgs_merge_plan_version_dev(arr, k, int(smallest_snapshot), lv, len(levels),
                                        int(max_grandparent_overlap_bytes), counts.data_ptr(),
                                        scr.data_ptr(), int(scr.numel()), sp),
          "lgs_merge_plan_version_dev")
    del alive
    cnt = [int(x) & _NO_RUN for x in counts.cpu()]
    if cnt[5] != _NO_RUN:
        e = MergeError(f"lgs_merge_plan_version_dev: run {cnt[5]} is not sorted or has a short key")
        e.rc, e.run = _native.LGS_EINVAL, cnt[5]
        raise e
    n, kb, vb, mk, dropped = cnt[:5]
    keys = torch.empty(kb + 16, dtype=torch.uint8, device=dev)
    vals = torch.empty(vb + 16, dtype=torch.uint8, device=dev)
    key_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    val_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    i32 = lambda: torch.empty(max(n, 1), dtype=torch.int32, device=dev)   # noqa: E731
    key_len, val_len, src_run, src_index, forced = i32(), i32(), i32(), i32(), i32()
    check(_L.lgs_merge_emit_dev(arr, k, n, keys.data_ptr(), key_off.data_ptr(),
                                key_len.data_ptr(), vals.data_ptr(), val_off.data_ptr(),
                                val_len.data_ptr(), src_run.data_ptr(), src_index.data_ptr(),
                                scr.data_ptr(), int(scr.numel()), sp), "lgs_merge_emit_dev")
    check(_L.lgs_merge_stops_dev(n_total, n, forced.data_ptr(), scr.data_ptr(), int(scr.numel()),
                                 sp), "lgs_merge_stops_dev")
    if stream is not None:
        scr.record_stream(stream)
    return {"keys": keys, "key_off": key_off, "key_len": key_len[:n], "vals": vals,
            "val_off": val_off, "val_len": val_len[:n], "src_run": src_run[:n],
            "src_index": src_index[:n], "n": n, "dropped": dropped, "key_bytes": kb,
            "val_bytes": vb, "max_key": mk, "forced": forced[:n], "n_forced": cnt[6]}


def merge_runs_host(runs, internal_keys: bool = False, drop: bool = False,
                    smallest_snapshot: int = 0, drop_deletions: bool = False, caps=None):
    """lgs_merge_host on lists of (key, value): returns ([(key, value)],
    [(run, index)], dropped).  caps: (entries, key bytes, value bytes) to call
    with; by default one call with nothing sizes the outputs.  Raises
    MergeError (``.rc``) where the call returns LGS_EINVAL or LGS_ENOSPC."""
    k = len(runs)
    arr = (_native.LgsRun * max(k, 1))()
    packed = []
    for r, run in enumerate(runs):
        a = _pack_entries(run)
        packed.append(a)
        arr[r] = _native.LgsRun(*(x.ctypes.data for x in a), len(run))
    needed = np.zeros(5, dtype=np.uint64)

    def call(n, kb, vb):
        out = (np.zeros(kb + 16, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64),
               np.zeros(max(n, 1), dtype=np.uint32), np.zeros(vb + 16, dtype=np.uint8),
               np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32),
               np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32))
        keys, koff, klen, vals, voff, vlen, srun, sidx = out
        rc = _L.lgs_merge_host(arr, k, 1 if internal_keys else 0, 1 if drop else 0,
                               int(smallest_snapshot), 1 if drop_deletions else 0,
                               keys.ctypes.data, kb, koff.ctypes.data, klen.ctypes.data,
                               vals.ctypes.data, vb, voff.ctypes.data, vlen.ctypes.data,
                               srun.ctypes.data, sidx.ctypes.data, n, needed.ctypes.data)
        return rc, out

    rc, out = call(*(caps if caps is not None else (0, 0, 0)))
    if rc == LGS_ENOSPC and caps is None:
        rc, out = call(*(int(x) for x in needed[:3]))
    if rc != _native.LGS_OK:
        msg = _L.lgs_last_error().decode(errors="replace")
        e = MergeError(f"lgs_merge_host failed ({rc}): {msg}")
        e.rc = rc
        e.needed = tuple(int(x) for x in needed)
        e.untouched = not any(a.any() for a in out)
        raise e
    n = int(needed[0])
    entries = _unpack_entries(*out[:6], n)
    return entries, [(int(out[6][i]), int(out[7][i])) for i in range(n)], int(needed[4])


_NO_SPLIT = (1 << 64) - 1


def build_tables_dev(run, block_size: int = 4096, restart_interval: int = 16,
                     compression: int = LGS_SNAPPY_COMPRESSION, bits_per_key: int = 0,
                     internal_keys: bool = False, max_file_size: int = _NO_SPLIT, stream=None,
                     forced=None):
    """The .ldb files a compaction writes for sorted entries in device memory,
    left in device memory (lgs_tables_build_dev): lcdb closes an output file
    once ldb_tablegen_size reaches ``max_file_size`` (db_impl.c:1417-1425);
    the default gives one file, ``build_table_host``'s image.

    ``run`` is a dict as ``merge_runs`` / ``block_entries`` return it (``keys``,
    ``key_off``, ``key_len``, ``vals``, ``val_off``, ``val_len`` and the ints
    ``n``, ``key_bytes``, ``val_bytes``).  Returns a dict: ``files`` (uint8,
    the images), ``file_off`` / ``file_size`` (int64, n_files), ``file_first``
    (int32, n_files + 1: file f holds entries file_first[f]:file_first[f+1])
    and the int ``n_files``.  No entries give no file.  The stream is drained
    when it returns.

    ``forced`` (int32 device tensor, one flag per entry, as
    ``merge_runs_version`` returns it) makes every flagged entry behind the
    first start a block and a file (lgs_tables_build_forced_dev): the files
    ldb_compaction_should_stop_before closes early.  None: no such starts."""
    import ctypes as C
    torch = _torch()
    n = int(run["n"]) if "n" in run else int(run["key_len"].numel())
    dev = run["keys"].device
    kb = int(run["key_bytes"]) if "key_bytes" in run else int(run["key_len"].sum())
    vb = int(run["val_bytes"]) if "val_bytes" in run else int(run["val_len"].sum())
    max_files = C.c_uint32(0)
    if forced is None:
        cap = int(_L.lgs_tables_build_bound(n, kb, vb, int(bits_per_key), int(max_file_size),
                                            C.byref(max_files)))
    else:
        if int(forced.numel()) < n:
            raise ValueError(f"{int(forced.numel())} forced flags for {n} entries")
        n_forced = int(run["n_forced"]) if "n_forced" in run else int((forced[:n] != 0).sum())
        cap = int(_L.lgs_tables_build_forced_bound(n, kb, vb, int(bits_per_key),
                                                   int(max_file_size), n_forced,
                                                   C.byref(max_files)))
    files = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
    nf_cap = max(int(max_files.value), 1)
    file_off = torch.zeros(nf_cap, dtype=torch.int64, device=dev)
    file_size = torch.zeros(nf_cap, dtype=torch.int64, device=dev)
    file_first = torch.zeros(nf_cap + 1, dtype=torch.int32, device=dev)
    nf, used = C.c_uint32(0), C.c_uint64(0)
    ptrs = [run[f].data_ptr() for f in ("keys", "key_off", "key_len", "vals", "val_off", "val_len")]
    head = (n, kb, vb, int(block_size), int(restart_interval), int(compression),
            int(bits_per_key), 1 if internal_keys else 0, int(max_file_size))
    tail = (files.data_ptr(), cap, file_off.data_ptr(), file_size.data_ptr(),
            file_first.data_ptr(), nf_cap, C.byref(nf), C.byref(used), _stream_ptr(stream))
    if forced is None:
        check(_L.lgs_tables_build_dev(*ptrs, *head, *tail), "lgs_tables_build_dev")
    else:
        check(_L.lgs_tables_build_forced_dev(*ptrs, *head, forced.data_ptr(), *tail),
              "lgs_tables_build_forced_dev")
    if stream is not None:
        for t in (files, file_off, file_size, file_first):
            t.record_stream(stream)
    f = int(nf.value)
    return {"files": files, "file_off": file_off[:f], "file_size": file_size[:f],
            "file_first": file_first[:f + 1], "n_files": f, "files_bytes": int(used.value)}


def _scan_runs(tables, bits_per_key, verify, opened):
    runs = []
    for img in tables:
        t = open_table(img, internal_keys=True, resident=True,
                       filter_name=FILTER_NAME if bits_per_key else None)
        opened.append(t)
        nxt = 0
        while True:
            r = t.scan_dev(first_block=nxt, max_blocks=65536, verify=verify)
            bad = r["index_status"] if r["at_end"] else LGS_ST_OK
            if bad == LGS_ST_OK and r["blocks_done"]:
                st = r["block_status"].cpu().numpy()
                bad = LGS_ST_OK if (st == LGS_ST_OK).all() else int(st[st != LGS_ST_OK][0])
            if bad != LGS_ST_OK:
                e = ScanError(f"compaction input ended with status {bad}")
                e.status = bad
                raise e
            runs.append(r)
            nxt = r["next_block"]
            if r["at_end"]:
                break
    return runs


def compact_to_files(tables, smallest_snapshot: int, drop_deletions: bool, block_size: int = 4096,
                     restart_interval: int = 16, compression: int = LGS_SNAPPY_COMPRESSION,
                     bits_per_key: int = 0, verify: bool = True,
                     max_output_file_size: int = 2 << 20):
    """One compaction's output files from its input table images, in the
    order ldb_inputiter_create hands them to the merging iterator (newest
    level-0 file first): ``OpenTable.scan_dev`` per table, ``merge_runs``
    with internal keys and the drop rule, ``build_tables_dev``; only the
    finished images and two keys per file come back to the host.

    ``drop_deletions`` is ldb_compaction_is_base_level_for_key for every key
    of the call; ``max_output_file_size`` is the compaction's
    (db_impl.c:1417-1425).  Neither depends on the levels below the output:
    ``compact_in_version`` takes those and applies
    ldb_compaction_should_stop_before and the per-key base level (DESIGN
    §4.10).  Returns one dict per file, in file order: ``image`` (bytes),
    ``smallest`` and ``largest`` (the internal keys of its first and last
    entry) and ``entries``: what ldb_edit_add_file takes.  No kept entry, no
    file."""
    return _compact_files(tables, bits_per_key, verify, lambda runs: merge_runs(
        runs, internal_keys=True, drop=True, smallest_snapshot=smallest_snapshot,
        drop_deletions=drop_deletions), block_size, restart_interval, compression,
        max_output_file_size)


def _compact_files(tables, bits_per_key, verify, merge, block_size, restart_interval, compression,
                   max_output_file_size):
    """scan -> ``merge(runs)`` -> build, and the files' rows for the host."""
    torch = _torch()
    opened = []
    try:
        runs = _scan_runs(tables, bits_per_key, verify, opened)
        m = merge(runs)
        b = build_tables_dev(m, block_size, restart_interval, compression, bits_per_key,
                             internal_keys=True, max_file_size=max_output_file_size,
                             forced=m.get("forced"))
        nf = b["n_files"]
        if nf == 0:
            return []
        first = b["file_first"].to(torch.int64)
        ends = torch.stack((first[:-1], first[1:] - 1), 1).reshape(-1)   # per file: first, last entry
        koff, klen = m["key_off"][ends], m["key_len"][ends].to(torch.int64)
        span = torch.arange(int(klen.max()), device=koff.device)
        at = (koff[:, None] + span[None, :]).clamp_(max=m["keys"].numel() - 1)
        keys, klen = m["keys"][at].cpu().numpy(), klen.cpu().numpy()
        off, size, first = (b[k].cpu().numpy() for k in ("file_off", "file_size", "file_first"))
        lo, hi = int(off[0]), int(off[-1] + size[-1])
        host = b["files"][lo:hi].cpu().numpy()
    finally:
        for t in opened:
            t.close()
    out = []
    for f in range(nf):
        at = int(off[f]) - lo
        out.append({"image": host[at:at + int(size[f])].tobytes(),
                    "smallest": keys[2 * f, :int(klen[2 * f])].tobytes(),
                    "largest": keys[2 * f + 1, :int(klen[2 * f + 1])].tobytes(),
                    "entries": int(first[f + 1]) - int(first[f])})
    return out


def compact_in_version(tables, smallest_snapshot: int, levels, block_size: int = 4096,
                       restart_interval: int = 16, compression: int = LGS_SNAPPY_COMPRESSION,
                       bits_per_key: int = 0, verify: bool = True,
                       max_output_file_size: int = 2 << 20,
                       max_grandparent_overlap_bytes: Optional[int] = None):
    """``compact_to_files`` for a compaction at level L of a version whose
    levels L + 2 .. 6 hold ``levels`` (a list of at most 5 lists of
    ``(smallest_ikey, largest_ikey, file_size)``, level L + 2 first, each in
    its level's order): lcdb's loop, db_impl.c:1352-1425, as lcdb runs it.

    ldb_compaction_should_stop_before closes the output file before a key
    once the file overlaps more than ``max_grandparent_overlap_bytes`` of
    ``levels[0]`` (None: 10 x ``max_output_file_size``, version_set.c:57), and
    a deletion is dropped where ldb_compaction_is_base_level_for_key holds
    for its user key.  Level L + 2 is given whole: files before the inputs are
    passed by the first key at no cost, files behind them are never reached,
    so the result is that of lcdb's overlapping subset.  Returns what
    ``compact_to_files`` returns."""
    limit = (10 * max_output_file_size if max_grandparent_overlap_bytes is None
             else max_grandparent_overlap_bytes)
    return _compact_files(tables, bits_per_key, verify, lambda runs: merge_runs_version(
        runs, smallest_snapshot, levels, limit), block_size, restart_interval, compression,
        max_output_file_size)


def compact_tables(tables, smallest_snapshot: int, drop_deletions: bool, block_size: int = 4096,
                   restart_interval: int = 16, compression: int = LGS_SNAPPY_COMPRESSION,
                   bits_per_key: int = 0, verify: bool = True) -> bytes:
    """One compaction's output as one table: ``compact_to_files`` with no
    limit on the output file's size (max_output_file_size is not applied, nor
    ldb_compaction_should_stop_before: see ``compact_in_version``), so scan, merge and build all stay
    in device memory and only the image is downloaded.  A compaction that
    keeps no entry gives lcdb's empty table, as ``build_table_host`` does."""
    files = compact_to_files(tables, smallest_snapshot, drop_deletions, block_size,
                             restart_interval, compression, bits_per_key, verify,
                             max_output_file_size=_NO_SPLIT)
    if not files:
        return build_table_host([], block_size, restart_interval, compression, bits_per_key,
                                internal_keys=True)
    return files[0]["image"]
