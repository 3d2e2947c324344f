"""Abort carry-over for TPC-C: the host-side rule and the C ABI's null checks.

A TPC-C access carries an 8-byte operation word beside its key, type and
table, so the rule of tests/test_carry.py -- the aborted txns of epoch k, in
sequence order, open epoch k + 1 ahead of fresh txns -- moves five arrays.
`host_carry` / `host_take` / `host_concat` restate it in numpy; the GPU tests
(tests/test_tpcc_closed_loop.py) run them around the oracle's TpccDB.epoch as
the reference of dv_tpcc_epoch_carry and dv_tpcc_epoch_run_closed_loop.
"""
import ctypes

import numpy as np

from dvcc import _lib as L
from dvcc.tpcc import TpccEpoch


def _gather_txns(tb, ids):
    """access indices of txns `ids` (in that order) of an epoch with
    txn_begin `tb`, and the new txn_begin"""
    lens = tb[ids + 1] - tb[ids]
    ntb = np.zeros(len(ids) + 1, np.int64)
    ntb[1:] = np.cumsum(lens)
    idx = np.repeat(tb[ids] - ntb[:-1], lens) + np.arange(int(ntb[-1]), dtype=np.int64)
    return idx, ntb.astype(np.uint32)


def _select(ep, ids):
    idx, ntb = _gather_txns(ep.txn_begin.astype(np.int64), np.asarray(ids, np.int64))
    return TpccEpoch(ep.keys[idx].copy(), ep.types[idx].copy(), ntb, ep.tables[idx].copy(), ep.args[idx].copy())


def host_carry(ep, commit, max_txn):
    """The aborted txns of `ep` (commit byte 0), in order, at most max_txn."""
    return _select(ep, np.flatnonzero(commit[:ep.n_txn] == 0)[:max_txn])


def host_take(pool, cur, n):
    """txns [cur, cur + n) of the pool, wrapping around it"""
    return _select(pool, (cur + np.arange(n)) % pool.n_txn)


def host_concat(a, b):
    tb = np.concatenate([a.txn_begin, b.txn_begin[1:] + a.txn_begin[-1]]).astype(np.uint32)
    return TpccEpoch(np.concatenate([a.keys, b.keys]), np.concatenate([a.types, b.types]), tb,
                     np.concatenate([a.tables, b.tables]), np.concatenate([a.args, b.args]))


def _hand_made():
    # 4 txns of 2, 1, 3, 1 accesses; args = op << 56 | operand
    args = (np.array([1, 2, 3, 4, 5, 5, 0], np.uint64) << np.uint64(56)) | np.arange(10, 17, dtype=np.uint64)
    return TpccEpoch(np.array([7, 1 << 40, 9, 3, 4, 5, 6], np.uint64), np.array([1, 1, 1, 1, 1, 1, 0], np.uint8),
                     np.array([0, 2, 3, 6, 7], np.uint32), np.array([0, 1, 2, 1, 4, 4, 3], np.uint8), args)


def test_host_carry_rule_with_args():
    ep = _hand_made()
    c = host_carry(ep, np.array([1, 0, 0, 1], np.uint8), 8)
    assert c.n_txn == 2 and list(c.txn_begin) == [0, 1, 4]
    assert list(c.keys) == [9, 3, 4, 5] and list(c.types) == [1, 1, 1, 1] and list(c.tables) == [2, 1, 4, 4]
    assert list(c.args) == list(ep.args[2:6])
    one = host_carry(ep, np.array([1, 0, 0, 1], np.uint8), 1)  # the cap cuts inside the aborted set
    assert one.n_txn == 1 and list(one.args) == [ep.args[2]] and list(one.tables) == [2]
    none = host_carry(ep, np.ones(4, np.uint8), 8)
    assert none.n_txn == 0 and none.n_acc == 0 and len(none.args) == 0
    t = host_take(ep, 3, 3)  # wraps: txns 3, 0, 1
    assert list(t.txn_begin) == [0, 1, 3, 4] and list(t.keys) == [6, 7, 1 << 40, 9]
    assert list(t.args) == [ep.args[6], ep.args[0], ep.args[1], ep.args[2]] and list(t.tables) == [3, 0, 1, 2]
    nxt = host_concat(c, t)
    assert nxt.n_txn == 5 and list(nxt.txn_begin) == [0, 1, 4, 5, 7, 8]
    assert list(nxt.args) == list(c.args) + list(t.args) and list(nxt.acc_txn()) == [0, 1, 1, 1, 2, 3, 3, 4]


def test_new_entry_points_reject_null_contexts():
    """dv_tpcc_epoch_carry / dv_tpcc_epoch_run_closed_loop with a null
    context: DV_ERR_ARG before any device is touched"""
    lib = L.lib()
    ep, out = L.EpochDev(), L.EpochDev()
    assert lib.dv_tpcc_epoch_carry(None, ctypes.byref(ep), None, 4, ctypes.byref(out), None) == L.DV_ERR_ARG
    bufs = (L.EpochDev * 2)()
    args = (ctypes.c_void_p * 2)()
    assert lib.dv_tpcc_epoch_run_closed_loop(None, ctypes.byref(ep), None, None, None, 4, bufs, args, 132, 1, 0,
                                             None, None, None) == L.DV_ERR_ARG
