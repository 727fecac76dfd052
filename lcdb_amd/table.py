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
    "index_host", "FILTER_NAME", "seek_blocks_host", "get_host", "open_table", "OpenTable", "build_blocks", "build_blocks_host", "build_table_host",
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


def open_table(file, paranoid_checks: bool = False, internal_keys: bool = False,
               filter_name: str | None = FILTER_NAME, resident: bool = False) -> OpenTable:
    """ldb_table_open once (lgs_table_open_host).  With ``resident=False`` the
    image is borrowed: pass a numpy uint8 array and keep it unchanged in its
    data blocks while the table is open (bytes are copied once instead)."""
    return OpenTable(file, paranoid_checks, internal_keys, filter_name, resident)
