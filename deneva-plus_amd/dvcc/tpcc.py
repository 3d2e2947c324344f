"""TPC-C on the engine (config E): loader, epoch builder and the per-epoch call.

Mirrors TPCCWorkload (benchmarks/tpcc_wl.cpp), TPCCQueryGenerator
(tpcc_query.cpp:26-263) and TPCCTxnManager's Payment / NewOrder
(tpcc_txn.cpp:117-244, 500-933) through libdvcc (dv_tpcc_*).  Decisions and
table state equal one worker thread running the epoch in sequence order
(SURVEY.md 8.0); inserted ORDER / NEW_ORDER / ORDER_LINE rows are determined by
the query, the commit byte and the o_id this path returns.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .engine import CCEngine, ClosedLoopBufs, DeviceEpoch, Epoch, LoopBackoff, _commit_ptrs, _ptr

TABLES = {"WAREHOUSE": L.T_WAREHOUSE, "DISTRICT": L.T_DISTRICT, "CUSTOMER": L.T_CUSTOMER,
          "ITEM": L.T_ITEM, "STOCK": L.T_STOCK, "CUST_LAST": L.T_CUST_LAST}


def tpcc_params(num_wh, dist_per_wh=10, cust_per_dist=3000, max_items=100000, max_items_per_txn=15,
                part_cnt=1, part_per_txn=2, wh_update=1, perc_payment=0.5, mpr=1.0):
    """g_* knobs (config.h:181-223; config E: PERC_PAYMENT 0.5, MPR 1.0)."""
    return L.TpccParams(num_wh, dist_per_wh, cust_per_dist, max_items, max_items_per_txn, part_cnt,
                        part_per_txn, wh_update, perc_payment, mpr)


@dataclass
class TpccEpoch(Epoch):
    args: np.ndarray = None      # uint64 [n_acc] op << 56 | operand
    txn_type: np.ndarray = None  # uint8 [n_txn] 1 Payment, 2 NewOrder
    owner: np.ndarray = None     # uint8 [n_acc] partition that runs the access


def table_rows(p, table, part_id=0):
    n = ctypes.c_uint64()
    L.check(L.lib().dv_tpcc_table_rows(ctypes.byref(p), part_id, table, ctypes.byref(n)), "dv_tpcc_table_rows")
    return n.value


def table(p, seed, table_id, part_id=0):
    """keys and the three state columns of one table as loaded (dv_tpcc_table)."""
    n = table_rows(p, table_id, part_id)
    out = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
    L.check(L.lib().dv_tpcc_table(ctypes.byref(p), seed, part_id, table_id, *[_ptr(a) for a in out]),
            "dv_tpcc_table")
    return out


def gen(p, n_txn, seed, home_part=0):
    cap = n_txn * (3 + 2 * p.max_items_per_txn)
    keys = np.zeros(cap, dtype=np.uint64)
    types = np.zeros(cap, dtype=np.uint8)
    tables = np.zeros(cap, dtype=np.uint8)
    args = np.zeros(cap, dtype=np.uint64)
    tb = np.zeros(n_txn + 1, dtype=np.uint32)
    tt = np.zeros(n_txn, dtype=np.uint8)
    own = np.zeros(cap, dtype=np.uint8)
    L.check(L.lib().dv_tpcc_gen(ctypes.byref(p), seed, home_part, n_txn, _ptr(keys), _ptr(types),
                                _ptr(tables), _ptr(args), _ptr(tb), _ptr(tt), _ptr(own)), "dv_tpcc_gen")
    n = int(tb[-1])
    return TpccEpoch(keys[:n].copy(), types[:n].copy(), tb, tables[:n].copy(), args[:n].copy(), tt,
                     own[:n].copy())


class TpccLoopBufs(ClosedLoopBufs):
    """The TPC-C closed loop's two epoch buffers (dv_tpcc_epoch_run_closed_loop):
    ClosedLoopBufs with table bytes (never the tb form), and the operation
    words of each buffer's accesses."""

    def __init__(self, cap, device):
        import torch
        super().__init__(cap, True, device)
        self.args = [torch.empty(max(1, self.cap), dtype=torch.int64, device=device) for _ in range(2)]

    def swap(self):
        super().swap()
        self.args.reverse()

    def epoch(self, b, n_txn, max_txn_acc):
        """buffer b's epoch as (DeviceEpoch, args) (reads its access count)"""
        dep = super().epoch(b, n_txn, max_txn_acc)
        return dep, self.args[b][:dep.n_acc]


class TpccLoopBackoff(LoopBackoff):
    """Exponential back-off for the TPC-C closed loops
    (dv_tpcc_closed_loop_backoff, dv_tpcc_closed_loop_backoff_lanes):
    LoopBackoff over a LoopTrack of two buffers (TpccEngine.closed_loop) or of
    2 L (TpccEngine.closed_loop_lanes over L contexts: one ring, shared by the
    lanes), attached to a TpccEngine -- the first of the lanes -- through the
    entry its loop accepts.  A released txn's accesses come from the pool
    again with their table bytes and operation words.  swap() (the single
    loop only) goes with TpccLoopBufs.swap and LoopTrack.swap after a call of
    n_epochs odd.  lanes says which loop the ring is for: a tracker of any
    other size than 2 * lanes is a ValueError (the single loop's ring is never
    built over a lanes tracker by accident)."""

    def __init__(self, track, n_slots, slot_cap=None, device="cuda", lanes=1):
        if lanes < 1 or track.n_bufs != 2 * lanes:
            raise ValueError("TpccLoopBackoff: a tracker of two buffers, or of 2 * lanes with lanes=")
        super().__init__(track, n_slots, slot_cap, device)

    def _entry(self, desc):
        if self.n_lanes == 1:
            L.check(L.lib().dv_tpcc_closed_loop_backoff(self.engine._ctx, desc), "dv_tpcc_closed_loop_backoff")
        else:
            L.check(L.lib().dv_tpcc_closed_loop_backoff_lanes(self.engine._ctx, desc, self.n_lanes),
                    "dv_tpcc_closed_loop_backoff_lanes")

    def _attach(self):
        arr = (ctypes.c_void_p * len(self.aborts))(*[int(t.data_ptr()) for t in self.aborts])
        d = L.LoopBackoffDesc(self.n_slots, self.slot_cap, self.park_ids.data_ptr(), self.park_aborts.data_ptr(),
                              self.slot_count.data_ptr(), arr, self.ctr.data_ptr())
        self._entry(ctypes.byref(d))

    def detach(self):
        if self.engine is not None:
            self._entry(None)
            self.engine._backoff = None
            self.engine = None


class TpccEngine(CCEngine):
    """A DV_TPCC context: the six tables of one partition in HBM."""

    def __init__(self, cc_alg, params, max_txn, device=0, part_id=0, seed=1, **kw):
        max_acc = max_txn * (3 + 2 * params.max_items_per_txn)
        super().__init__(cc_alg, max_txn, max_acc, device=device, part_cnt=params.part_cnt,
                         part_id=part_id, workload=L.TPCC, **kw)
        self.params = params
        L.check(L.lib().dv_tpcc_load(self._ctx, ctypes.byref(params), seed), "dv_tpcc_load")

    def read_col(self, table_id, col, first=0, n=None):
        if n is None:
            n = table_rows(self.params, table_id, self.part_id) - first
        out = np.zeros(n, dtype=np.uint64)
        L.check(L.lib().dv_read_table_col(self._ctx, table_id, col, first, n, _ptr(out)), "dv_read_table_col")
        return out

    def begin_tpcc(self, dep, d_args, d_oid=None):
        """Staged form (partitioned epochs): rounds and finish as CCEngine's."""
        self._after_torch()
        self._desc = dep.desc()
        self._keep = (d_args, d_oid)  # alive until finish
        L.check(L.lib().dv_tpcc_epoch_begin(self._ctx, ctypes.byref(self._desc), _ptr(d_args), _ptr(d_oid)),
                "dv_tpcc_epoch_begin")

    def run_tpcc_epoch_device(self, dep, d_args, d_commit, d_oid=None):
        self._after_torch()
        st = L.Stats()
        L.check(L.lib().dv_tpcc_epoch_run_device(self._ctx, ctypes.byref(dep.desc()), _ptr(d_args),
                                                 _ptr(d_commit), _ptr(d_oid), ctypes.byref(st)),
                "dv_tpcc_epoch_run_device")
        return st


    def run_tpcc_epochs_device(self, deps, d_args, d_commits=None, d_oids=None, lanes=None):
        """Several TPC-C epochs back to back (dv_tpcc_epoch_run_device_batch):
        epoch k+1 is queued before epoch k is read back.  deps / d_args: one
        DeviceEpoch and operation-word tensor per epoch; d_commits / d_oids:
        one device tensor per epoch, one tensor for all, or None.  lanes:
        decision lanes (open_lane) -- dv_tpcc_epoch_run_device_lanes over
        [self] + lanes.  Returns the list of stats."""
        ctxs = [self] + list(lanes or [])
        for e in ctxs:
            e._after_torch()
        n = len(deps)

        def ptrs(x):
            if x is None:
                return None
            xs = x if isinstance(x, (list, tuple)) else [x] * n
            return (ctypes.c_void_p * n)(*[_ptr(t) for t in xs])
        descs = (L.EpochDev * n)(*[d.desc() for d in deps])
        args = ptrs(list(d_args))
        sts = (L.Stats * n)()
        self._keep = (deps, d_args, d_commits, d_oids)
        if len(ctxs) > 1:
            lp = (ctypes.c_void_p * len(ctxs))(*[e._ctx.value for e in ctxs])
            L.check(L.lib().dv_tpcc_epoch_run_device_lanes(lp, len(ctxs), descs, args, n, ptrs(d_commits),
                                                           ptrs(d_oids), sts), "dv_tpcc_epoch_run_device_lanes")
        else:
            L.check(L.lib().dv_tpcc_epoch_run_device_batch(self._ctx, descs, args, n, ptrs(d_commits),
                                                           ptrs(d_oids), sts), "dv_tpcc_epoch_run_device_batch")
        return list(sts)

    def carry(self, dep, d_args, max_txn=None):
        """Abort carry-over (dv_tpcc_epoch_carry): the last epoch's (`dep`'s,
        with operation words d_args) aborted txns, in sequence order, at most
        max_txn of them, as (DeviceEpoch, args)."""
        import torch
        dev = dep.keys.device
        n = max(1, dep.n_acc)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        types = torch.empty(n, dtype=torch.uint8, device=dev)
        txn = torch.empty(n, dtype=torch.int32, device=dev)
        tabs = torch.empty(n, dtype=torch.uint8, device=dev)
        args = torch.empty(n, dtype=torch.int64, device=dev)
        out = L.EpochDev(keys.data_ptr(), types.data_ptr(), txn.data_ptr(), tabs.data_ptr(), 0, 0, 0)
        cap = dep.n_txn if max_txn is None else max_txn
        self._after_torch()
        L.check(L.lib().dv_tpcc_epoch_carry(self._ctx, ctypes.byref(dep.desc()), _ptr(d_args), cap,
                                            ctypes.byref(out), _ptr(args)), "dv_tpcc_epoch_carry")
        n = int(out.n_acc)
        return (DeviceEpoch.from_tensors(keys[:n], types[:n], txn[:n], int(out.n_txn), tables=tabs[:n],
                                         max_txn_acc=int(out.max_txn_acc)), args[:n])

    def closed_loop(self, pool, pool_args, pool_begin, n_txn, n_epochs, cursor=None, bufs=None, d_commits=None,
                    d_oids=None, resume=False, track=None):
        """The TPC-C closed loop on the device (dv_tpcc_epoch_run_closed_loop):
        n_epochs epochs of n_txn txns, each the previous one's aborted txns
        (with their operation words) then fresh ones from `pool` (a DeviceEpoch
        with tables and max_txn_acc > 0; pool_args: its operation words;
        pool_begin: its n_txn + 1 access offsets, int32 device tensor) from the
        device word `cursor` (int32 tensor, advanced).  bufs: TpccLoopBufs
        (allocated when None); d_commits / d_oids: a device tensor per epoch,
        one for all, or None.  track: a LoopTrack attached to this engine.  A
        TpccLoopBackoff attached to this engine (after its tracker) backs the
        retries off; it needs no argument here.
        Returns (stats list, bufs, cursor); the next epoch is in
        bufs.epoch(n_epochs & 1): after an odd call TpccLoopBufs.swap,
        LoopTrack.swap and TpccLoopBackoff.swap go together, in that order."""
        track = self._tracked(track, n_txn, 2)
        cursor, sts = self._loop_state(pool, cursor, n_epochs)
        if bufs is None:
            bufs = TpccLoopBufs(n_txn * pool.max_txn_acc, pool.keys.device)
        arr = (L.EpochDev * 2)(*[bufs.desc(b) for b in range(2)])
        bargs = getattr(bufs, "args", None) or [None, None]
        aps = (ctypes.c_void_p * 2)(*[(int(t.data_ptr()) if t is not None else None) for t in bargs])
        n = len(sts)
        self._after_torch()
        L.check(L.lib().dv_tpcc_epoch_run_closed_loop(self._ctx, ctypes.byref(pool.desc()), _ptr(pool_args),
                                                      _ptr(pool_begin), _ptr(cursor), n_txn, arr, aps, bufs.cap,
                                                      n_epochs, int(resume), _commit_ptrs(d_commits, n),
                                                      _commit_ptrs(d_oids, n), sts),
                "dv_tpcc_epoch_run_closed_loop")
        if track is not None:
            track.done += n_epochs
        return list(sts)[:n_epochs], bufs, cursor

    def closed_loop_lanes(self, lanes, pool, pool_args, pool_begin, n_txn, n_epochs, cursor=None, bufs=None,
                          d_commits=None, d_oids=None, resume=False, track=None):
        """dv_tpcc_epoch_run_closed_loop_lanes over [self] + lanes
        (open_lane): epoch k on context k % L, each context's epochs a TPC-C
        closed loop of their own (aborted txns, with their operation words,
        retried L epochs later), the pool cursor shared, executions in epoch
        order.  bufs: one TpccLoopBufs per context (allocated when None).
        track: a LoopTrack of 2 L buffers attached to this engine (with a
        TpccLoopBackoff built over it and attached too, a txn's a-th abort
        costs L - 1 + min(2^(a-1), D) epochs).  Returns (stats list, bufs,
        cursor); resume needs the previous call's n_epochs to be a multiple
        of 2 L."""
        ctxs = [self] + list(lanes)
        nl = len(ctxs)
        track = self._tracked(track, n_txn, 2 * nl)
        cursor, sts = self._loop_state(pool, cursor, n_epochs)
        if bufs is None:
            bufs = [TpccLoopBufs(n_txn * pool.max_txn_acc, pool.keys.device) for _ in range(nl)]
        arr = (L.EpochDev * (2 * nl))(*[b.desc(i) for b in bufs for i in range(2)])
        bargs = [t for b in bufs for t in (getattr(b, "args", None) or [None, None])]
        aps = (ctypes.c_void_p * (2 * nl))(*[(int(t.data_ptr()) if t is not None else None) for t in bargs])
        lp = (ctypes.c_void_p * nl)(*[e._ctx.value for e in ctxs])
        n = len(sts)
        for e in ctxs:
            e._after_torch()
        L.check(L.lib().dv_tpcc_epoch_run_closed_loop_lanes(lp, nl, ctypes.byref(pool.desc()), _ptr(pool_args),
                                                            _ptr(pool_begin), _ptr(cursor), n_txn, arr, aps,
                                                            bufs[0].cap, n_epochs, int(resume),
                                                            _commit_ptrs(d_commits, n), _commit_ptrs(d_oids, n), sts),
                "dv_tpcc_epoch_run_closed_loop_lanes")
        if track is not None:
            track.done += n_epochs
        return list(sts)[:n_epochs], bufs, cursor

    def run_tpcc_epoch_part(self, home, d_args, d_owner, txns_per_rank, d_commit, d_oid=None):
        """Config E from the engine (dv_tpcc_epoch_run_part): this rank's
        client batch `home` (DeviceEpoch), its operation words and owner
        bytes; d_commit / d_oid sized for the global epoch (ranks x
        txns_per_rank), d_oid equal on every rank afterwards."""
        self._after_torch()
        st = L.Stats()
        L.check(L.lib().dv_tpcc_epoch_run_part(self._ctx, ctypes.byref(home.desc()), _ptr(d_args), _ptr(d_owner),
                                               txns_per_rank, _ptr(d_commit), _ptr(d_oid), ctypes.byref(st)),
                "dv_tpcc_epoch_run_part")
        return st


def device_epoch(e, device="cuda"):
    """(DeviceEpoch, args tensor) of a TpccEpoch."""
    import torch
    dep = DeviceEpoch(e, device)
    return dep, torch.from_numpy(e.args.view(np.int64)).to(device)
