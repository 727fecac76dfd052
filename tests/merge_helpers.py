"""What the merge tests share (test_gpu_merge.py, test_gpu_merge_sweep.py,
merge_sweep.py): internal keys, the binary user keys, and the upload of runs
to the device and the download of a merge's result.  Nothing here touches the
GPU until it is called."""
from __future__ import annotations

import struct

import numpy as np


def ikey(user: bytes, seq: int, typ: int = 1) -> bytes:
    return user + struct.pack("<Q", (seq << 8) | typ)


def binary_users(rng, count: int):
    """`count` distinct user keys over the alphabet a, \\0, \\xff at lengths 0,
    1, 7, 8, 9, 15, 16 and 17: cuts of four base strings with up to two bytes
    changed, so that keys agree up to any position, differ in a byte before,
    in or behind the first 8, and are each other's prefixes padded with \\0."""
    alphabet = (0x61, 0x00, 0xff)
    bases = [bytes(rng.choice(alphabet) for _ in range(17)) for _ in range(4)]
    users = {b""}
    while len(users) < count:
        u = bytearray(rng.choice(bases)[:rng.choice((1, 7, 8, 9, 15, 16, 17))])
        for _ in range(rng.randrange(3)):
            u[rng.randrange(len(u))] = rng.choice(alphabet)
        users.add(bytes(u))
    return sorted(users)


def run_of(i: int, k: int) -> int:
    """Run r takes r + 1 of every 1 + 2 + ... + k entries."""
    x = (i * 7 + i // 5) % (k * (k + 1) // 2)
    return next(r for r in range(k) if x < (r + 1) * (r + 2) // 2)


def upload(tab, entries):
    """One run as device tensors, the dict block_entries / scan_dev return."""
    import torch
    dev = torch.device("cuda")
    keys, koff, klen, vals, voff, vlen = tab._pack_entries(entries)
    n = len(entries)
    koff = np.append(koff, np.uint64(klen.sum()))
    voff = np.append(voff, np.uint64(vlen.sum()))

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)

    return {"keys": up(keys, np.uint8), "key_off": up(koff, np.int64),
            "key_len": up(klen, np.int32) if n else torch.zeros(0, dtype=torch.int32, device=dev),
            "vals": up(vals, np.uint8), "val_off": up(voff, np.int64),
            "val_len": up(vlen, np.int32) if n else torch.zeros(0, dtype=torch.int32, device=dev),
            "n": n}


def download(tab, m):
    """([(key, value)], [(run, index)]) of a merge_runs result."""
    n = m["n"]
    es = tab._unpack_entries(m["keys"].cpu().numpy(), m["key_off"].cpu().numpy(),
                             m["key_len"].cpu().numpy().view(np.uint32), m["vals"].cpu().numpy(),
                             m["val_off"].cpu().numpy(),
                             m["val_len"].cpu().numpy().view(np.uint32), n)
    sr, si = m["src_run"].cpu().numpy(), m["src_index"].cpu().numpy()
    return es, [(int(sr[i]), int(si[i])) for i in range(n)]


def on_device(tab, runs, **kw):
    m = tab.merge_runs([upload(tab, r) for r in runs], **kw)
    es, src = download(tab, m)
    assert int(m["key_off"][m["n"]]) == m["key_bytes"] == sum(len(k) for k, _ in es)
    assert int(m["val_off"][m["n"]]) == m["val_bytes"] == sum(len(v) for _, v in es)
    assert m["max_key"] == max([len(k) for k, _ in es] or [0])
    return es, src, m["dropped"]


def both(tab, runs, **kw):
    """The host call and the device calls, which must agree; returns one."""
    h = tab.merge_runs_host(runs, **kw)
    d = on_device(tab, runs, **kw)
    assert h[0] == d[0] and h[1] == d[1] and h[2] == d[2]
    return h
