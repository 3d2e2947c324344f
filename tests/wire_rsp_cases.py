"""Test infrastructure for dv_wire_respond_device (the reply mbufs packed on
the device): the cases, an independent numpy packer written from the format
description in include/dvcc.h -- not from csrc/wire.cpp -- and the host
packer's (dv_wire_respond) output for a case, which is what the GPU tests
compare against.

A reply batch (include/dvcc.h, "Deneva wire format"): {u32 dest, u32 src,
u32 count}, then `count` messages back to back.  CL_RSP: rtype u32, txn_id
u64, mq_time u64, 7 latency doubles, client_startts u64 = 84 bytes.
CALVIN_ACK: rtype u32, txn_id u64, batch_id u64, mq_time u64, 7 latency
doubles, rc u32 = 88 bytes.  A batch is at most 4,096 bytes, so a full one
holds (4096 - 12) // 84 = 48 or (4096 - 12) // 88 = 46 messages.
Destinations ascend; a destination's messages keep txn (list) order.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from dvcc import _lib as L

HDR, MSG_MAX = 12, 4096
CL_RSP_T = np.dtype([("rtype", "<u4"), ("txn_id", "<u8"), ("mq", "<u8"), ("lat", "<f8", (7,)), ("cst", "<u8")])
ACK_T = np.dtype([("rtype", "<u4"), ("txn_id", "<u8"), ("batch_id", "<u8"), ("mq", "<u8"), ("lat", "<f8", (7,)),
                  ("rc", "<u4")])
assert CL_RSP_T.itemsize == 84 and ACK_T.itemsize == 88
NODE_ID = 3


def per(calvin):
    return (MSG_MAX - HDR) // (ACK_T if calvin else CL_RSP_T).itemsize


def field(t, salt):
    """a u64 per index whose eight bytes are all distinct (byte k carries k in
    its top three bits) and which is >= 2^32: a swapped half, a shifted byte
    or another txn's value cannot go unseen"""
    t = np.asarray(t, np.uint64)
    v = np.zeros(t.shape, np.uint64)
    for k in range(8):
        low = ((t >> np.uint64(5 * k)) ^ np.uint64((salt + 3 * k) & 31)) & np.uint64(31)
        v |= (np.uint64(k << 5) | low) << np.uint64(8 * k)
    return v


@dataclass
class Case:
    name: str
    calvin: bool
    n_dest: int
    rnode: np.ndarray            # uint32 [txns]
    commit: np.ndarray = None    # uint8 [txns] or None: every txn answered
    src: np.ndarray = None       # uint32 list or None
    batch_id: int = 0x1122334455667788

    def __post_init__(self):
        self.rnode = np.ascontiguousarray(self.rnode, np.uint32)
        n = len(self.rnode)
        self.txn_id, self.cst = field(np.arange(n), 1), field(np.arange(n), 9)
        if self.commit is not None:
            self.commit = np.ascontiguousarray(self.commit, np.uint8)
        if self.src is not None:
            self.src = np.ascontiguousarray(self.src, np.uint32)

    @property
    def n(self):
        return len(self.rnode) if self.src is None else len(self.src)

    @property
    def n_src_txn(self):
        return len(self.rnode) if self.src is not None else 0

    def answered(self):
        """the txns answered, in the order their replies are due"""
        if self.src is not None:
            return self.src.astype(np.int64)
        if self.commit is not None:
            return np.flatnonzero(self.commit)
        return np.arange(len(self.rnode))


def numpy_pack(c):
    """the reply batches (list of bytes) from the format description alone"""
    idx = c.answered()
    dest = c.rnode[idx]
    out = []
    for d in np.unique(dest):
        mine = idx[dest == d]  # (boolean selection keeps the order)
        m = np.zeros(len(mine), ACK_T if c.calvin else CL_RSP_T)
        m["rtype"] = L.WIRE_CALVIN_ACK if c.calvin else L.WIRE_CL_RSP
        m["txn_id"] = c.txn_id[mine]
        if c.calvin:
            m["batch_id"] = c.batch_id
        else:
            m["cst"] = c.cst[mine]
        for s in range(0, len(mine), per(c.calvin)):
            part = m[s:s + per(c.calvin)]
            out.append(np.array([d, NODE_ID, len(part)], "<u4").tobytes() + part.tobytes())
    return out


def cfg_of(c):
    return L.WireCfg(L.YCSB, 1 if c.calvin else 0, NODE_ID, 1, 1, 0, 0, None)


def host_pack(c, cap=None, max_batches=None):
    """dv_wire_respond over the case -> (status, bytes written as a uint8
    array, batch_off, n_batches).  A list and, under CALVIN (where the host
    packer acknowledges every txn), commit bytes are applied first: the packer
    then sees the answered txns' fields alone, every one committed."""
    idx = c.answered()
    tid, cst, rn = (np.ascontiguousarray(a[idx]) for a in (c.txn_id, c.cst, c.rnode))
    n = len(idx)
    e = L.WireEpoch()
    e.n_txn = e.max_txn = n
    e.batch_id = c.batch_id
    e.txn_id, e.return_node = tid.ctypes.data, rn.ctypes.data
    e.client_startts = None if c.calvin else cst.ctypes.data
    ones = np.ones(max(1, n), np.uint8)
    mb = n // per(c.calvin) + len(np.unique(rn)) + 1 if max_batches is None else max_batches
    cap = mb * MSG_MAX if cap is None else cap
    out, off = np.zeros(max(1, cap), np.uint8), np.zeros(mb + 1, np.uint64)
    nb = ctypes.c_uint32()
    cfg = cfg_of(c)
    rc = L.lib().dv_wire_respond(ctypes.byref(cfg), ctypes.byref(e), ones.ctypes.data, out.ctypes.data, cap,
                                 off.ctypes.data, mb, ctypes.byref(nb))
    if rc != L.DV_OK:
        return rc, None, None, 0
    return rc, out[:int(off[nb.value])], off[:nb.value + 1], nb.value


def split(buf, off, nb):
    return [bytes(buf[int(off[b]):int(off[b + 1])]) for b in range(nb)]


TILE = 256


def cases(calvin):
    """every case of the issue for one dialect, by name"""
    rng = np.random.default_rng(46 if calvin else 48)
    p = per(calvin)
    out = []

    def add(name, n_dest, rnode, commit=None, src=None):
        out.append(Case(name, calvin, n_dest, rnode, commit, src))

    def some(n, frac=0.7):
        """commit bytes for a CL_RSP case; an ack case answers every txn"""
        return None if calvin else (rng.random(n) < frac).astype(np.uint8) * 3

    for n in (0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1):  # the tile edges
        add(f"tile_n{n}", 3, rng.integers(0, 3, n), some(n))
    for k in (p - 1, p, p + 1, 2 * p, 2 * p + 1):  # the mbuf edges
        add(f"one_dest_{k}", 4, np.full(k, 2))
    add("n_dest_1", 1, np.zeros(300), some(300))
    add("n_dest_256_one_each", 256, rng.permutation(256))
    add("dest_0_and_255", 256, rng.choice([0, 255], 600), some(600))
    add("alternating", 2, np.arange(700) % 2, some(700, 0.9))
    add("change_at_tile_boundary", 2, np.r_[np.ones(2 * TILE), np.zeros(TILE), np.ones(TILE + 76)])
    add("commit_none", 3, rng.integers(0, 3, 500), np.zeros(500))
    add("commit_all", 3, rng.integers(0, 3, 500), np.ones(500))
    lanes = np.zeros(3 * TILE + 1, np.uint8)
    for t0 in range(0, len(lanes), TILE):
        lanes[[t for t in (t0, t0 + 63, t0 + 64, t0 + 255) if t < len(lanes)]] = 1
    add("commit_lanes_0_63_64_255", 2, rng.integers(0, 2, len(lanes)), lanes)
    add("random_70000", 5, rng.integers(0, 5, 70_000), some(70_000, 0.6))
    add("src_permutation", 4, rng.integers(0, 4, 600), src=rng.permutation(600))
    add("src_repeats", 4, rng.integers(0, 4, 600), src=rng.integers(0, 600, 900))
    add("src_empty", 4, rng.integers(0, 4, 600), src=np.zeros(0))
    return out


ALL = {(c.name, c.calvin): c for cal in (False, True) for c in cases(cal)}
IDS = [f"{'ack' if cal else 'rsp'}-{name}" for name, cal in ALL]
