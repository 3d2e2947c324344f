"""Deneva wire format in and out of the engine (include/dvcc.h, dv_wire_*).

A server node's ingress of its clients' message batches -- the mbufs runcl's
MessageThread sends (transport/msg_thread.cpp:53-111): CL_QRY messages of
YCSBClientQueryMessage / TPCCClientQueryMessage (transport/message.cpp:
451-687, 856-916), or under CALVIN the sequencer's forwarded CL_QRY batches
ended by RDONE -- decoded by libdvcc straight into the host arrays of an
epoch, and the replies (CL_RSP to the clients, CALVIN_ACK to the sequencers)
packed the same way from the epoch's commit bytes.  DeviceWireIngress does
the YCSB ingress on the device instead (dv_wire_ingest_device): the receive
queue's bytes in, a device-resident epoch out.  TpccDeviceWireIngress does the
same for TPC-C client batches (dv_wire_ingest_device_tpcc), every message
expanded to its access list on the device.  CalvinDeviceWireIngress takes
CALVIN sequencer streams (dv_wire_ingest_device_calvin, YCSB): cut at the
message where the batch id changes, appended stream by stream in node order;
CalvinTpccDeviceWireIngress the same streams of TPC-C queries
(dv_wire_ingest_device_calvin_tpcc).  No combination of workload and CALVIN is
left on the host decoder.  The device ingresses also answer on the device:
respond_device / respond_logged_device pack the reply mbufs there
(dv_wire_respond_device) and return device tensors; reply_batches slices a
host copy of them into respond's list of batches.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .engine import DeviceEpoch, Epoch, _ptr


@dataclass
class WireEpoch(Epoch):
    """An epoch decoded from batches, with what the replies need."""
    args: np.ndarray = None            # TPC-C operation words
    txn_type: np.ndarray = None        # TPC-C: 1 Payment, 2 NewOrder
    owner: np.ndarray = None           # partition of every access
    txn_id: np.ndarray = None          # uint64 [n_txn]
    client_startts: np.ndarray = None  # uint64 [n_txn]
    return_node: np.ndarray = None     # uint32 [n_txn]: client (CALVIN: sequencer)
    batch_id: int = None               # CALVIN
    rdone: int = 0                     # CALVIN: RDONEs taken for batch_id


def _pack_replies(cfg, n, batch_id, txn_id, client_startts, return_node, commit):
    """The host packer (dv_wire_respond) over n txns' reply fields (host
    arrays; client_startts None under CALVIN, whose acks carry none) -> the
    reply batches (bytes) of the txns whose commit byte is set, of every txn
    when commit is None."""
    tid, rn = np.ascontiguousarray(txn_id, np.uint64), np.ascontiguousarray(return_node, np.uint32)
    cst = None if client_startts is None else np.ascontiguousarray(client_startts, np.uint64)
    e = L.WireEpoch()
    e.n_txn, e.max_txn = n, n
    e.batch_id = L.WIRE_NO_BATCH_ID if batch_id is None else batch_id
    e.txn_id, e.return_node = tid.ctypes.data, rn.ctypes.data
    e.client_startts = None if cst is None else cst.ctypes.data
    # a reply: the header (Message::mget_size, message.cpp:196-209), then client_startts or the ack's result;
    # a batch holds (MSG_MAX - 12) // its size of them; one partial batch per destination
    msg = 4 + 8 + (8 if cfg.calvin else 0) + 8 + 7 * 8 + (4 if cfg.calvin else 8)
    max_b = n // ((L.WIRE_MSG_MAX - L.WIRE_HDR) // msg) + len(np.unique(rn)) + 1
    out = np.zeros(max_b * L.WIRE_MSG_MAX, np.uint8)
    off = np.zeros(max_b + 1, np.uint64)
    nb = ctypes.c_uint32()
    L.check(L.lib().dv_wire_respond(ctypes.byref(cfg), ctypes.byref(e), _ptr(commit), _ptr(out), len(out),
                                    _ptr(off), max_b, ctypes.byref(nb)), "dv_wire_respond")
    return [out[int(off[b]):int(off[b + 1])].tobytes() for b in range(nb.value)]


def reply_batches(out, batch_off, n_batches):
    """What respond_device / respond_logged_device return (device tensors, or
    host copies of them) as the list of batches (bytes) respond returns.
    Device tensors are copied once the device is idle: they are written on
    the engine's stream, which torch's copy does not wait for."""
    if getattr(out, "is_cuda", False):
        import torch
        torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)  # noqa: E731
    buf, off = h(out).view(np.uint8), h(batch_off).view(np.uint64)
    return [buf[int(off[b]):int(off[b + 1])].tobytes() for b in range(n_batches)]


class WireIngress:
    """dv_wire_open / dv_wire_decode / dv_wire_respond over host buffers of
    max_txn txns and max_acc accesses.  feed(batch) decodes a received batch
    (bytes); whenever the current epoch cannot take the next message (full,
    or a CALVIN message of a later batch) it is closed and queued, and
    decoding goes on into a fresh one.  take() closes the current epoch
    early; ready holds the closed ones."""

    def __init__(self, workload, max_txn, max_acc, node_id=0, node_cnt=1, part_cnt=1, synth_table_size=0,
                 calvin=False, tpcc=None, max_req=0):
        self.cfg = L.WireCfg(workload, 1 if calvin else 0, node_id, node_cnt, part_cnt, max_req, synth_table_size,
                             ctypes.pointer(tpcc) if tpcc is not None else None)
        self._tpcc = tpcc
        self.workload = workload
        self.max_txn, self.max_acc = max_txn, max_acc
        self.ready = []
        self._bufs = self._alloc()
        self.ep = L.WireEpoch()
        self._bind()
        L.check(L.lib().dv_wire_epoch_reset(ctypes.byref(self.ep)), "dv_wire_epoch_reset")

    def _alloc(self):
        tp = self.workload == L.TPCC
        A, T = self.max_acc, self.max_txn
        return dict(keys=np.zeros(A, np.uint64), types=np.zeros(A, np.uint8), txn_begin=np.zeros(T + 1, np.uint32),
                    tables=np.zeros(A, np.uint8) if tp else None, args=np.zeros(A, np.uint64) if tp else None,
                    txn_type=np.zeros(T, np.uint8) if tp else None, owner=np.zeros(A, np.uint8),
                    txn_id=np.zeros(T, np.uint64), client_startts=np.zeros(T, np.uint64),
                    return_node=np.zeros(T, np.uint32))

    def _bind(self):
        self.ep.max_txn, self.ep.max_acc = self.max_txn, self.max_acc
        for k, v in self._bufs.items():
            setattr(self.ep, k, None if v is None else v.ctypes.data)

    def _close(self):
        b, e = self._bufs, self.ep
        n, a = e.n_txn, e.n_acc
        cut = lambda x, m: None if x is None else x[:m].copy()  # noqa: E731
        out = WireEpoch(cut(b["keys"], a), cut(b["types"], a), b["txn_begin"][:n + 1].copy(),
                        cut(b["tables"], a), args=cut(b["args"], a), txn_type=cut(b["txn_type"], n),
                        owner=cut(b["owner"], a), txn_id=cut(b["txn_id"], n),
                        client_startts=cut(b["client_startts"], n), return_node=cut(b["return_node"], n),
                        batch_id=None if e.batch_id == (1 << 64) - 1 else int(e.batch_id), rdone=int(e.rdone))
        L.check(L.lib().dv_wire_epoch_reset(ctypes.byref(e)), "dv_wire_epoch_reset")
        return out

    def feed(self, batch):
        """Decodes one received batch; returns the epochs it closed."""
        buf = np.frombuffer(bytes(batch), dtype=np.uint8)
        cur = L.WireCursor()
        L.check(L.lib().dv_wire_open(ctypes.byref(self.cfg), _ptr(buf), len(buf), ctypes.byref(cur)), "dv_wire_open")
        closed = []
        while True:
            rc = L.lib().dv_wire_decode(ctypes.byref(self.cfg), ctypes.byref(cur), ctypes.byref(self.ep))
            if rc == L.WIRE_MORE:
                closed.append(self._close())
                continue
            L.check(rc, "dv_wire_decode")
            break
        self.ready.extend(closed)
        return closed

    def feed_many(self, batches):
        """Decodes a list of received batches with one call per epoch
        (dv_wire_decode_batches); returns the epochs it closed."""
        if not batches:
            return []
        off = np.zeros(len(batches) + 1, np.uint64)
        off[1:] = np.cumsum([len(b) for b in batches])
        buf = np.frombuffer(b"".join(bytes(b) for b in batches), dtype=np.uint8)
        return self.feed_buffer(buf, off)

    def feed_buffer(self, buf, off):
        """The same over batches already back to back in one uint8 array,
        batch b at buf[off[b]:off[b + 1]]."""
        cur = L.WireCursor()
        nxt = ctypes.c_uint32(0)
        closed = []
        while True:
            rc = L.lib().dv_wire_decode_batches(ctypes.byref(self.cfg), _ptr(buf), _ptr(off), len(off) - 1,
                                                ctypes.byref(cur), ctypes.byref(nxt), ctypes.byref(self.ep))
            if rc == L.WIRE_MORE:
                closed.append(self._close())
                continue
            L.check(rc, "dv_wire_decode_batches")
            break
        self.ready.extend(closed)
        return closed

    def take(self):
        """Closes and returns the epoch being filled."""
        return self._close()

    def respond(self, ep, commit=None):
        """The replies to a decoded epoch as a list of batches (bytes):
        CL_RSP for every committed txn (commit bytes), or under CALVIN a
        CALVIN_ACK for every txn."""
        n = ep.n_txn
        cm = None if commit is None else np.ascontiguousarray(np.asarray(commit)[:n], np.uint8)
        return _pack_replies(self.cfg, n, ep.batch_id, ep.txn_id, ep.client_startts, ep.return_node, cm)


class _DeviceIngress:
    """What the device ingresses share: the engine whose context and stream
    they work on, the cfg, the capacities, the device (_dev) and the tensors
    every dialect fills -- txn_begin and the reply fields txn_id /
    client_startts / return_node."""

    def __init__(self, engine, cfg, max_txn, max_acc, device):
        import torch
        self.engine, self.cfg, self._dev = engine, cfg, device
        self.max_txn, self.max_acc = int(max_txn), int(max_acc)
        self.txn_begin = self._new(self.max_txn + 1, torch.int32)
        self.txn_id, self.client_startts = self._new(self.max_txn, torch.int64), self._new(self.max_txn, torch.int64)
        self.return_node = self._new(self.max_txn, torch.int32)

    def _new(self, n, dtype):
        import torch
        return torch.empty(n, dtype=dtype, device=self._dev)

    def _new_accesses(self, *dtypes):
        """a tensor of max_acc elements (one at least) per dtype"""
        return [self._new(max(1, self.max_acc), dt) for dt in dtypes]

    @staticmethod
    def _upload(buf, off, device):
        """numpy bytes / offsets as the device tensors the entry points take"""
        import torch
        if isinstance(buf, np.ndarray):
            buf = torch.from_numpy(np.ascontiguousarray(buf, np.uint8)).to(device)
        if isinstance(off, np.ndarray):
            off = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).to(device)
        return buf, off

    @staticmethod
    def _check(rc, launched, what):
        """raises unless the kernels ran and decided rc: a call refused before
        any launch (launched False: its result record untouched) or a HIP failure"""
        if rc not in (L.DV_OK, L.WIRE_MORE, L.DV_ERR_ARG) or not launched:
            L.check(rc, what)

    n_dest = L.WIRE_DEST_MAX  # every return node lies below it (set it lower for smaller reply buffers)

    def _respond_device(self, n, commit, src, n_src_txn, txn_id, client_startts, return_node, batch_id=None):
        """dv_wire_respond_device over device reply fields -> (out, batch_off,
        n_batches): the reply mbufs back to back in a uint8 device tensor, batch
        b at out[batch_off[b]:batch_off[b + 1]] (int64 device tensor).  The
        tensors are the ingress's own, sized for n replies to n_dest
        destinations and written on the engine's stream: the next call
        overwrites them."""
        import torch
        calvin = bool(self.cfg.calvin)
        msg = 4 + 8 + (8 if calvin else 0) + 8 + 7 * 8 + (4 if calvin else 8)
        max_b = n // ((L.WIRE_MSG_MAX - L.WIRE_HDR) // msg) + self.n_dest + 1
        cap = max_b * L.WIRE_HDR + n * msg
        if getattr(self, "_rsp_out", None) is None or self._rsp_out.numel() < cap:
            self._rsp_out = self._new(cap, torch.uint8)
        if getattr(self, "_rsp_off", None) is None or self._rsp_off.numel() < max_b + 1:
            self._rsp_off = self._new(max_b + 1, torch.int64)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        rin = L.WireRspIn(n, self.n_dest, p(commit), p(src), n_src_txn, 0, p(txn_id), p(client_startts),
                          p(return_node), L.WIRE_NO_BATCH_ID if batch_id is None else batch_id)
        rout = L.WireRspOut(self._rsp_out.data_ptr(), cap, self._rsp_off.data_ptr(), max_b, 0)
        res = L.WireRspResult(status=1)
        self.engine._after_torch()
        rc = L.lib().dv_wire_respond_device(self.engine._ctx, ctypes.byref(self.cfg), ctypes.byref(rin),
                                            ctypes.byref(rout), ctypes.byref(res))
        L.check(rc, "dv_wire_respond_device")  # (a return node at or above n_dest: DV_ERR_ARG)
        self._rsp_held = (commit, src)  # (the emit may still read them when this returns)
        return self._rsp_out[:res.n_bytes], self._rsp_off[:res.n_batches + 1], res.n_batches

    def _with_replies(self, ep, n):
        """ep with the device reply arrays of its n txns"""
        ep.txn_id, ep.client_startts, ep.return_node = self.txn_id[:n], self.client_startts[:n], self.return_node[:n]
        return ep


class _DeviceReplies(_DeviceIngress):
    """The CL_RSP replies of an epoch of client batches ingested on the
    device, whatever the workload (DeviceWireIngress, TpccDeviceWireIngress)."""

    def respond(self, ep, d_commit):
        """The CL_RSP batches (bytes) of the epoch's committed txns (d_commit:
        device commit bytes): their reply fields compacted on the device, then
        the host packer (dv_wire_respond) over them."""
        import torch
        n = ep.n_txn
        tid = torch.empty(max(1, n), dtype=torch.int64, device=self._dev)
        cst = torch.empty(max(1, n), dtype=torch.int64, device=self._dev)
        rn = torch.empty(max(1, n), dtype=torch.int32, device=self._dev)
        cnt = ctypes.c_uint32()
        self.engine._after_torch()
        L.check(L.lib().dv_wire_reply_fields_device(self.engine._ctx, d_commit.data_ptr(), n, ep.txn_id.data_ptr(),
                                                    ep.client_startts.data_ptr(), ep.return_node.data_ptr(),
                                                    tid.data_ptr(), cst.data_ptr(), rn.data_ptr(),
                                                    ctypes.byref(cnt)), "dv_wire_reply_fields_device")
        return self._pack(tid, cst, rn, cnt.value)

    def respond_device(self, ep, d_commit):
        """respond's batches packed on the device (dv_wire_respond_device):
        (out, batch_off, n_batches) as _respond_device returns them --
        reply_batches(out, batch_off, n_batches) is respond(ep, d_commit)."""
        return self._respond_device(ep.n_txn, d_commit, None, 0, ep.txn_id, ep.client_startts, ep.return_node)

    def respond_logged_device(self, src):
        """respond_logged's batches packed on the device: the reply fields of
        the epoch this ingress decoded last are read through `src` by the
        packer itself, in list order."""
        import torch
        idx = src.to(device=self.txn_id.device, dtype=torch.int32).contiguous()
        return self._respond_device(int(idx.numel()), None, idx, self.max_txn, self.txn_id, self.client_startts,
                                    self.return_node)

    def _pack(self, tid, cst, rn, c):
        """the host packer (dv_wire_respond) over the first c entries of device
        reply fields, every one committed"""
        if not c:
            return []
        h = lambda t, dt: t[:c].cpu().numpy().view(dt)  # noqa: E731
        return _pack_replies(self.cfg, c, None, h(tid, np.uint64), h(cst, np.uint64), h(rn, np.uint32),
                             np.ones(c, np.uint8))

    def respond_logged(self, src):
        """The CL_RSP batches (bytes) of the pool txns `src` names: a slice of
        a closed loop's commit log (LoopTrack.commits(i)[0], an integer device
        tensor of indices into the epoch this ingress decoded last, which the
        loop ran as its pool).  Their reply fields are gathered by index on the
        device, then packed as respond packs its compacted ones -- a server
        answering at commit, whatever epoch a txn committed in."""
        import torch
        idx = src.to(device=self.txn_id.device, dtype=torch.int64)
        c = int(idx.numel())
        if not c:
            return []
        self.engine._after_torch()
        return self._pack(self.txn_id[idx], self.client_startts[idx], self.return_node[idx], c)


class TpccDeviceWireIngress(_DeviceReplies):
    """dv_wire_ingest_device_tpcc over device buffers of max_txn txns and
    max_acc accesses on `engine`'s context: a receive queue's TPC-C CL_QRY
    batches into a DeviceEpoch with tables, whole batches at a time, the
    access lists following `params` (dv_tpcc_params; the engine's own when it
    is a TpccEngine running the epoch).  respond / respond_logged pack the
    replies.  The epoch's tensors are the ingress's own: the next feed_buffer
    overwrites them."""

    def __init__(self, engine, params, max_txn, max_acc, node_id=0, node_cnt=1, part_cnt=1, device="cuda"):
        import torch
        super().__init__(engine, L.WireCfg(L.TPCC, 0, node_id, node_cnt, part_cnt, 0, 0, ctypes.pointer(params)),
                         max_txn, max_acc, device)
        self.params = params
        self.next_txn = 0
        self.n_acc_dev = self._new(1, torch.int32)
        self.keys, self.types, self.acc_txn = self._new_accesses(torch.int64, torch.uint8, torch.int32)
        self.tables, self.args, self.owner = self._new_accesses(torch.uint8, torch.int64, torch.uint8)
        self.txn_type = self._new(self.max_txn, torch.uint8)

    def feed_buffer(self, buf, off, first_batch=0):
        """Batches first_batch.. of buf (a torch uint8 device tensor, or a numpy
        array, uploaded) at offsets off (u64 [n + 1], numpy or an int64 device
        tensor) -> (epoch, n_taken, status), status as DeviceWireIngress's.
        The epoch (DeviceEpoch with tables, of exact size) is written on the
        engine's stream and carries args (its operation words), txn_begin,
        txn_type, owner and the device reply arrays: run it with
        run_tpcc_epoch_device(ep, ep.args, ...), or hand it to closed_loop as
        the pool (ep, ep.args, ep.txn_begin)."""
        buf, off = self._upload(buf, off, self._dev)
        self.engine._after_torch()
        p = lambda t: t.data_ptr()  # noqa: E731
        out = L.WireTpccDevOut(self.max_txn, 0, self.max_acc, p(self.txn_begin), p(self.n_acc_dev), p(self.keys),
                               p(self.types), p(self.acc_txn), p(self.tables), p(self.args), p(self.txn_type),
                               p(self.owner), p(self.txn_id), p(self.client_startts), p(self.return_node))
        res = L.WireDevResult()
        rc = L.lib().dv_wire_ingest_device_tpcc(self.engine._ctx, ctypes.byref(self.cfg), buf.data_ptr(), buf.numel(),
                                                off.data_ptr(), off.numel() - 1, first_batch, ctypes.byref(out),
                                                self.next_txn, ctypes.byref(res))
        self._check(rc, res.status == rc, "dv_wire_ingest_device_tpcc")
        self._held = (buf, off)  # (the decode may still read them when this returns)
        self.next_txn = res.next_txn
        n, a = res.n_txn, res.n_acc
        ep = DeviceEpoch.from_tensors(self.keys[:a], self.types[:a], self.acc_txn[:a], n, tables=self.tables[:a],
                                      max_txn_acc=res.max_txn_acc)
        ep.args, ep.owner = self.args[:a], self.owner[:a]
        ep.txn_begin, ep.txn_type = self.txn_begin[:n + 1], self.txn_type[:n]
        return self._with_replies(ep, n), res.n_taken, res.status


class DeviceWireIngress(_DeviceReplies):
    """dv_wire_ingest_device / dv_wire_reply_fields_device over device
    buffers of max_txn txns and max_acc accesses on `engine`'s context (YCSB,
    NO_WAIT / WAIT_DIE / OCC).  feed_buffer decodes a receive queue's batches
    into a DeviceEpoch, whole batches at a time; respond packs the replies of
    its committed txns.  The epoch's tensors are the ingress's own: the next
    feed_buffer overwrites them."""

    def __init__(self, engine, max_txn, max_acc, node_id=0, node_cnt=1, part_cnt=1, synth_table_size=0, max_req=0,
                 device="cuda"):
        import torch
        super().__init__(engine, L.WireCfg(L.YCSB, 0, node_id, node_cnt, part_cnt, max_req, synth_table_size, None),
                         max_txn, max_acc, device)
        self.next_txn = 0
        self.n_acc_dev = self._new(1, torch.int32)
        # 4-byte records hold keys below 2^31 (dv_epoch_dev::recs32)
        self.recs32 = self._new_accesses(torch.int32)[0] if synth_table_size <= 1 << 31 else None
        self.keys = self.types = self.acc_txn = None  # (allocated by the first epoch that needs them)

    def _old_form(self):
        import torch
        if self.keys is None:
            self.keys, self.types, self.acc_txn = self._new_accesses(torch.int64, torch.uint8, torch.int32)

    def _ingest(self, buf, off, first_batch, old):
        out = L.WireDevOut(self.max_txn, 0, self.max_acc, self.txn_begin.data_ptr(), self.n_acc_dev.data_ptr(),
                           self.recs32.data_ptr() if self.recs32 is not None else None,
                           self.keys.data_ptr() if old else None, self.types.data_ptr() if old else None,
                           self.acc_txn.data_ptr() if old else None, None, self.txn_id.data_ptr(),
                           self.client_startts.data_ptr(), self.return_node.data_ptr())
        res = L.WireDevResult()
        rc = L.lib().dv_wire_ingest_device(self.engine._ctx, ctypes.byref(self.cfg), buf.data_ptr(), buf.numel(),
                                           off.data_ptr(), off.numel() - 1, first_batch, ctypes.byref(out),
                                           self.next_txn, ctypes.byref(res))
        self._check(rc, res.status == rc, "dv_wire_ingest_device")
        return res

    def feed_buffer(self, buf, off, first_batch=0):
        """Batches first_batch.. of buf (a torch uint8 device tensor, or a numpy
        array, uploaded) at offsets off (u64 [n + 1], numpy or an int64 device
        tensor) -> (epoch, n_taken, status).  status DV_OK: all taken;
        WIRE_MORE: the epoch is full, call again with first_batch = n_taken;
        DV_ERR_ARG: batch n_taken is malformed (or alone exceeds the
        capacity); the epoch holds the batches before it.  The epoch is
        written on the engine's stream (run it there; other streams
        synchronise first) and carries the device reply arrays."""
        buf, off = self._upload(buf, off, self._dev)
        self.engine._after_torch()
        # records and boundaries alone when the epoch takes the tb-mode prefix
        # path, both forms otherwise -- as loop_form picks for the closed loop.
        # The path depends on the epoch's size, known once it is decoded: a
        # short last epoch is decoded again with both forms.
        old = self.recs32 is None or not self.engine.reads_tb_only(self.max_txn)
        if old:
            self._old_form()
        res = self._ingest(buf, off, first_batch, old)
        if not old and not self.engine.reads_tb_only(res.n_txn):
            old = True
            self._old_form()
            res = self._ingest(buf, off, first_batch, old)
        self._held = (buf, off)  # (the decode may still read them when this returns)
        self.next_txn = res.next_txn
        n, a = res.n_txn, res.n_acc
        if self.recs32 is not None:
            ep = DeviceEpoch.from_device_buffers(self.recs32, self.txn_begin, self.n_acc_dev, n, a, res.max_txn_acc,
                                                 self.keys if old else None, self.types if old else None,
                                                 self.acc_txn if old else None)
        else:
            ep = DeviceEpoch.from_tensors(self.keys[:a], self.types[:a], self.acc_txn[:a], n,
                                          max_txn_acc=res.max_txn_acc)
        return self._with_replies(ep, n), res.n_taken, res.status


class _CalvinStreams(_DeviceIngress):
    """Sequencer streams, cut at message granularity, appended into one open
    epoch, whatever the workload (CalvinDeviceWireIngress,
    CalvinTpccDeviceWireIngress): the cursor and the epoch's totals between
    calls, sequence() and the CALVIN_ACK replies.  A subclass names its entry
    point (_entry), builds the call's out (_out) and the epoch (_epoch)."""

    _entry = None

    def __init__(self, engine, cfg, max_txn, max_acc, device):
        super().__init__(engine, cfg, max_txn, max_acc, device)
        self._held = []
        self.status = L.DV_OK
        self._open()

    def _open(self):
        """an empty epoch: no txn, no batch id yet"""
        self.n_txn = self.n_acc = self.rdone = self.max_txn_acc = 0
        self.batch_id = None

    def feed_buffer(self, buf, off, pos=None):
        """Appends one sequencer's stream -- mbufs back to back in buf (a torch
        uint8 device tensor, or a numpy array, uploaded) at offsets off (u64
        [n + 1]) -- to the open epoch, from the cursor pos: None for the
        stream's start, a (mbuf, message) pair, or the WireCalvinPos an
        earlier call returned.  Returns the updated WireCalvinPos: the new
        cursor, the epoch's totals and `stop`, why the call ended
        (WIRE_STOP_END: the stream is consumed; BATCH: the message at the
        cursor opens the next batch -- take() the epoch once every sequencer's
        stream got there; CAPACITY: the epoch is full; MALFORMED / STALE: the
        mbuf / message at the cursor is refused).  self.status holds the C
        status.  A window's end (WIRE_STOP_WINDOW) is called again here."""
        buf, off = self._upload(buf, off, self._dev)
        self.engine._after_torch()
        p = L.WireCalvinPos()
        if pos is not None:
            p.batch, p.msg = (pos.batch, pos.msg) if isinstance(pos, L.WireCalvinPos) else pos
        p.n_txn, p.rdone, p.n_acc, p.max_txn_acc = self.n_txn, self.rdone, self.n_acc, self.max_txn_acc
        p.batch_id = L.WIRE_NO_BATCH_ID if self.batch_id is None else self.batch_id
        out = self._out()
        entry = getattr(L.lib(), self._entry)
        while True:
            p.stop = 0xFFFFFFFF
            rc = entry(self.engine._ctx, ctypes.byref(self.cfg), buf.data_ptr(), buf.numel(), off.data_ptr(),
                       off.numel() - 1, ctypes.byref(out), ctypes.byref(p))
            self._check(rc, p.stop != 0xFFFFFFFF, self._entry)
            if p.stop != L.WIRE_STOP_WINDOW:
                break
        self._held.append((buf, off))  # (the decode may still read them when this returns)
        self.status = rc
        self.n_txn, self.rdone, self.n_acc, self.max_txn_acc = p.n_txn, p.rdone, p.n_acc, p.max_txn_acc
        self.batch_id = None if p.batch_id == L.WIRE_NO_BATCH_ID else int(p.batch_id)
        return p

    def take(self):
        """Closes the open epoch and returns it: a DeviceEpoch of exact size
        over the ingress's tensors (written on the engine's stream: run it
        there), with batch_id, rdone (one per sequencer when the batch is
        complete), txn_begin and the device reply arrays."""
        n, a = self.n_txn, self.n_acc
        ep = self._epoch(n, a)
        ep.batch_id, ep.rdone = self.batch_id, self.rdone
        ep.txn_begin = self.txn_begin[:n + 1]
        self._with_replies(ep, n)
        self._held = self._held[-2:]
        self._open()
        return ep

    def sequence(self, streams, cursors=None):
        """One Calvin epoch from every sequencer's stream: streams is [(buf,
        off)] in node order, cursors where each stands (None: all at their
        start).  Every stream is fed up to the end of its batch (BATCH) or of
        its bytes (END); anything else raises.  Returns (epoch, cursors), the
        cursors for the next batch."""
        cursors = [None] * len(streams) if cursors is None else list(cursors)
        nxt = []
        for (buf, off), cur in zip(streams, cursors):
            p = self.feed_buffer(buf, off, cur)
            if p.stop not in (L.WIRE_STOP_BATCH, L.WIRE_STOP_END):
                raise L.DvccError(self.status, f"{self._entry}: stop {p.stop} at mbuf {p.batch}, "
                                               f"message {p.msg}")
            nxt.append((p.batch, p.msg))
        return self.take(), nxt

    def respond(self, ep):
        """The CALVIN_ACK batches (bytes) of the epoch, one ack per txn to its
        sequencer: every txn is acknowledged, so the reply fields go to the
        host packer (dv_wire_respond) as they are."""
        n = ep.n_txn
        if not n:
            return []
        self.engine._after_torch()
        return _pack_replies(self.cfg, n, ep.batch_id, ep.txn_id.cpu().numpy().view(np.uint64), None,
                             ep.return_node.cpu().numpy().view(np.uint32), None)

    def respond_device(self, ep):
        """respond's batches packed on the device (dv_wire_respond_device):
        (out, batch_off, n_batches) as _respond_device returns them --
        reply_batches(out, batch_off, n_batches) is respond(ep)."""
        return self._respond_device(ep.n_txn, None, None, 0, ep.txn_id, None, ep.return_node, ep.batch_id)


class CalvinDeviceWireIngress(_CalvinStreams):
    """dv_wire_ingest_device_calvin over device buffers of max_txn txns and
    max_acc accesses on `engine`'s context (YCSB under CALVIN): sequencer
    streams, cut at message granularity, appended into one open epoch.  An
    epoch is one sequencer batch per sequencer in origin-major order:
    feed_buffer once per stream, in node order (or sequence(), which does
    that), then take().  The epoch's tensors are the ingress's own: the feeds
    after the next take() overwrite them."""

    _entry = "dv_wire_ingest_device_calvin"

    def __init__(self, engine, max_txn, max_acc, node_id=0, node_cnt=1, part_cnt=1, synth_table_size=0, max_req=0,
                 device="cuda"):
        import torch
        super().__init__(engine, L.WireCfg(L.YCSB, 1, node_id, node_cnt, part_cnt, max_req, synth_table_size, None),
                         max_txn, max_acc, device)
        self.keys, self.types, self.acc_txn = self._new_accesses(torch.int64, torch.uint8, torch.int32)

    def _out(self):
        q = lambda t: t.data_ptr()  # noqa: E731
        return L.WireDevOut(self.max_txn, 0, self.max_acc, q(self.txn_begin), None, None, q(self.keys), q(self.types),
                            q(self.acc_txn), None, q(self.txn_id), q(self.client_startts), q(self.return_node))

    def _epoch(self, n, a):
        return DeviceEpoch.from_tensors(self.keys[:a], self.types[:a], self.acc_txn[:a], n,
                                        max_txn_acc=self.max_txn_acc)


class CalvinTpccDeviceWireIngress(_CalvinStreams):
    """dv_wire_ingest_device_calvin_tpcc over device buffers of max_txn txns
    and max_acc accesses on `engine`'s context (TPC-C under CALVIN): what
    CalvinDeviceWireIngress does for a sequencer's TPC-C stream, every CL_QRY
    expanded to its access list following `params` (dv_tpcc_params; the
    engine's own when it is a TpccEngine running the epoch).  take() returns a
    DeviceEpoch with tables that also carries args (its operation words),
    owner and txn_type: run it with run_tpcc_epoch_device(ep, ep.args, ...)."""

    _entry = "dv_wire_ingest_device_calvin_tpcc"

    def __init__(self, engine, params, max_txn, max_acc, node_id=0, node_cnt=1, part_cnt=1, device="cuda"):
        import torch
        super().__init__(engine, L.WireCfg(L.TPCC, 1, node_id, node_cnt, part_cnt, 0, 0, ctypes.pointer(params)),
                         max_txn, max_acc, device)
        self.params = params
        self.keys, self.types, self.acc_txn = self._new_accesses(torch.int64, torch.uint8, torch.int32)
        self.tables, self.args, self.owner = self._new_accesses(torch.uint8, torch.int64, torch.uint8)
        self.txn_type = self._new(self.max_txn, torch.uint8)

    def _out(self):
        q = lambda t: t.data_ptr()  # noqa: E731
        return L.WireTpccDevOut(self.max_txn, 0, self.max_acc, q(self.txn_begin), None, q(self.keys), q(self.types),
                                q(self.acc_txn), q(self.tables), q(self.args), q(self.txn_type), q(self.owner),
                                q(self.txn_id), q(self.client_startts), q(self.return_node))

    def _epoch(self, n, a):
        ep = DeviceEpoch.from_tensors(self.keys[:a], self.types[:a], self.acc_txn[:a], n, tables=self.tables[:a],
                                      max_txn_acc=self.max_txn_acc)
        ep.args, ep.owner, ep.txn_type = self.args[:a], self.owner[:a], self.txn_type[:n]
        return ep


def _seq_cfg(node_id, node_cnt, part_cnt, synth_table_size, max_req, params=None):
    """the sequencer's cfg: YCSB, or TPC-C following `params` (a TpccParams,
    which the caller keeps alive as long as the cfg points at it)"""
    if params is None:
        return L.WireCfg(L.YCSB, 1, node_id, node_cnt, part_cnt, max_req, synth_table_size, None)
    return L.WireCfg(L.TPCC, 1, node_id, node_cnt, part_cnt, 0, 0, ctypes.pointer(params))


def _seq_room(in_bytes, node_cnt):
    """(cap, max_batches) that the fan-out of in_bytes of client mbufs cannot
    pass: every message to every node, two consecutive mbufs of a destination
    hold more than 4,084 message bytes, an RDONE and a last mbuf per node."""
    msgs = in_bytes * node_cnt
    max_b = 2 * msgs // (L.WIRE_MSG_MAX - L.WIRE_HDR) + 2 * node_cnt
    return msgs + 84 * node_cnt + L.WIRE_HDR * max_b, max_b


_ACK_MSG, _SEQ_RSP_MSG = 88, 92  # AckMessage, ClientResponseMessage of a CALVIN build


def _seq_rsp_room(n, n_dest):
    """(cap, max_batches) for n CL_RSPs to n_dest destinations"""
    max_b = n // ((L.WIRE_MSG_MAX - L.WIRE_HDR) // _SEQ_RSP_MSG) + min(n, n_dest) + 1
    return max_b * L.WIRE_HDR + n * _SEQ_RSP_MSG, max_b


@dataclass
class SequencedBatch:
    """What dv_wire_sequence wrote (host arrays at their full capacity):
    mbuf j at out[batch_off[j]:batch_off[j + 1]], destination d's mbufs
    dest_first[d] .. dest_first[d + 1] - 1, the wait list's first n_txn
    entries, and the result record."""
    out: np.ndarray
    batch_off: np.ndarray
    dest_first: np.ndarray
    wait_client: np.ndarray
    wait_startts: np.ndarray
    wait_acks: np.ndarray
    result: object

    def mbufs(self, dest=None):
        """the outgoing mbufs (bytes), all or one destination's"""
        lo, hi = (0, self.result.n_out) if dest is None else (int(self.dest_first[dest]), int(self.dest_first[dest + 1]))
        return [self.out[int(self.batch_off[j]):int(self.batch_off[j + 1])].tobytes() for j in range(lo, hi)]


def sequence_host(buf, off, batch_id, *, node_id, node_cnt, part_cnt, synth_table_size=0, n_dest, max_txn, max_req=0,
                  first_batch=0, cap=None, max_batches=None, params=None):
    """dv_wire_sequence over numpy arrays: the client mbufs first_batch.. of
    buf (uint8) at offsets off (u64 [n + 1]) stamped as batch batch_id of
    sequencer node_id and fanned out -> SequencedBatch.  cap / max_batches
    default to what the input cannot pass.  With `params` (a TpccParams) the
    mbufs are TPC-C's, YCSB's otherwise.  A call the library refuses before
    it looks at the bytes raises; result.status holds every other outcome."""
    buf, off = np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64)
    blen = len(buf)
    if not blen:
        buf = np.zeros(1, np.uint8)  # (an empty queue still has an address)
    cfg = _seq_cfg(node_id, node_cnt, part_cnt, synth_table_size, max_req, params)  # (params: alive to the return)
    room = _seq_room(blen, node_cnt)
    cap, max_b = room[0] if cap is None else cap, room[1] if max_batches is None else max_batches
    b = SequencedBatch(np.zeros(max(cap, 4), np.uint8), np.zeros(max_b + 1, np.uint64),
                       np.zeros(node_cnt + 1, np.uint32), np.zeros(max(1, max_txn), np.uint32),
                       np.zeros(max(1, max_txn), np.uint64), np.zeros(max(1, max_txn), np.uint32),
                       L.WireSeqResult(status=-1000))
    sin = L.WireSeqIn(buf.ctypes.data, blen, off.ctypes.data, len(off) - 1, first_batch, batch_id, n_dest, max_txn)
    sout = L.WireSeqOut(b.out.ctypes.data, cap, b.batch_off.ctypes.data, max_b, 0, b.dest_first.ctypes.data,
                        b.wait_client.ctypes.data, b.wait_startts.ctypes.data, b.wait_acks.ctypes.data)
    rc = L.lib().dv_wire_sequence(ctypes.byref(cfg), ctypes.byref(sin), ctypes.byref(sout), ctypes.byref(b.result))
    if b.result.status != rc:
        L.check(rc, "dv_wire_sequence")
    return b


def sequence_acks_host(buf, off, batch_id, wait_client, wait_startts, wait_acks, *, node_id, node_cnt, n_dest,
                       part_cnt=1, cap=None, max_batches=None, params=None):
    """dv_wire_sequence_acks over numpy arrays: the ack mbufs of buf / off
    counted against batch batch_id's wait list (wait_acks, uint32, is updated
    in place) -> (out, batch_off, result), the CL_RSP mbufs of the txns that
    completed at out[batch_off[j]:batch_off[j + 1]], j < result.n_batches.
    With `params` (a TpccParams) the cfg is TPC-C's; the acks are the same."""
    buf, off = np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(off, np.uint64)
    blen = len(buf)
    if not blen:
        buf = np.zeros(1, np.uint8)
    assert wait_acks.dtype == np.uint32 and wait_acks.flags.c_contiguous
    wc, ws = np.ascontiguousarray(wait_client, np.uint32), np.ascontiguousarray(wait_startts, np.uint64)
    n = len(wait_acks)
    cfg = _seq_cfg(node_id, node_cnt, part_cnt, 0, 0, params)
    room = _seq_rsp_room(n, n_dest)
    cap, max_b = room[0] if cap is None else cap, room[1] if max_batches is None else max_batches
    out, boff = np.zeros(max(cap, 4), np.uint8), np.zeros(max_b + 1, np.uint64)
    ain = L.WireSeqAckIn(buf.ctypes.data, blen, off.ctypes.data, len(off) - 1, n_dest, batch_id, n, 0,
                         wc.ctypes.data, ws.ctypes.data, wait_acks.ctypes.data)
    rout = L.WireRspOut(out.ctypes.data, cap, boff.ctypes.data, max_b, 0)
    res = L.WireSeqAckResult(status=-1000)
    rc = L.lib().dv_wire_sequence_acks(ctypes.byref(cfg), ctypes.byref(ain), ctypes.byref(rout), ctypes.byref(res))
    if res.status != rc:
        L.check(rc, "dv_wire_sequence_acks")
    return out, boff, res


class DeviceSequencer:
    """The CALVIN sequencer of node node_id on `engine`'s context and stream
    (dv_wire_sequence_device / dv_wire_sequence_acks_device): YCSB client
    mbufs, or TPC-C's following `params` (a TpccParams) when given.  It owns
    the wait list of the batch it sequenced last (wait_client, wait_startts,
    wait_acks: device tensors of max_txn entries, n_txn of them live) and the
    output tensors, which the next call of the same kind overwrites.  cap /
    max_batches bound the outgoing bytes and mbufs of sequence(); by default
    they are what the call's input cannot pass."""

    def __init__(self, engine, node_id, node_cnt, part_cnt, synth_table_size, max_req, max_txn, n_dest, cap=None,
                 max_batches=None, device="cuda", params=None):
        import torch
        self.engine, self._dev = engine, device
        self.params = params  # (the cfg points at it)
        self.cfg = _seq_cfg(node_id, node_cnt, part_cnt, synth_table_size, max_req, params)
        self.node_id, self.node_cnt, self.n_dest, self.max_txn = node_id, node_cnt, n_dest, int(max_txn)
        self.cap, self.max_batches = cap, max_batches
        new = lambda n, dt: torch.zeros(max(1, n), dtype=dt, device=device)  # noqa: E731
        self.wait_client, self.wait_acks = new(self.max_txn, torch.int32), new(self.max_txn, torch.int32)
        self.wait_startts = new(self.max_txn, torch.int64)
        self.dest_first = new(node_cnt + 1, torch.int32)
        self.batch_id, self.n_txn = None, 0
        self._out = self._off = self._rsp_out = self._rsp_off = None

    def _grown(self, t, n, dtype):
        import torch
        return t if t is not None and t.numel() >= n else torch.empty(n, dtype=dtype, device=self._dev)

    def sequence(self, buf, off, batch_id, first_batch=0):
        """The client mbufs first_batch.. of buf (a torch uint8 device tensor,
        or a numpy array, uploaded) at offsets off become batch batch_id ->
        (out, batch_off, dest_first, result): device tensors written on the
        engine's stream, of exact size where the call wrote them, and the
        result record (status DV_OK, WIRE_MORE: call again from n_taken for
        the next batch, or DV_ERR_ARG)."""
        import torch
        buf, off = _DeviceIngress._upload(buf, off, self._dev)
        room = _seq_room(buf.numel(), self.node_cnt)
        cap, max_b = room[0] if self.cap is None else self.cap, room[1] if self.max_batches is None else self.max_batches
        self._out = self._grown(self._out, max(cap, 4), torch.uint8)
        self._off = self._grown(self._off, max_b + 1, torch.int64)
        sin = L.WireSeqIn(buf.data_ptr(), buf.numel(), off.data_ptr(), off.numel() - 1, first_batch, batch_id,
                          self.n_dest, self.max_txn)
        sout = L.WireSeqOut(self._out.data_ptr(), cap, self._off.data_ptr(), max_b, 0, self.dest_first.data_ptr(),
                            self.wait_client.data_ptr(), self.wait_startts.data_ptr(), self.wait_acks.data_ptr())
        res = L.WireSeqResult(status=-1000)
        self.engine._after_torch()
        rc = L.lib().dv_wire_sequence_device(self.engine._ctx, ctypes.byref(self.cfg), ctypes.byref(sin),
                                             ctypes.byref(sout), ctypes.byref(res))
        _DeviceIngress._check(rc, res.status == rc, "dv_wire_sequence_device")
        self._held = (buf, off)  # (the emit may still read them when this returns)
        wrote = res.status != L.DV_ERR_ARG or (res.n_bytes <= cap and res.n_out <= max_b)
        self.batch_id, self.n_txn = (batch_id, res.n_txn) if wrote else (None, 0)
        if not wrote:
            return self._out[:0], self._off[:0], self.dest_first[:0], res
        return self._out[:res.n_bytes], self._off[:res.n_out + 1], self.dest_first, res

    def acks(self, buf, off):
        """The ack mbufs of buf / off counted against the wait list ->
        (out, batch_off, n_batches, result): the CL_RSP mbufs of the txns whose
        last ack came, as respond_device returns its replies."""
        import torch
        if self.batch_id is None:
            raise L.DvccError(L.DV_ERR_ARG, "DeviceSequencer.acks: no batch sequenced")
        buf, off = _DeviceIngress._upload(buf, off, self._dev)
        cap, max_b = _seq_rsp_room(self.n_txn, self.n_dest)
        self._rsp_out = self._grown(self._rsp_out, max(cap, 4), torch.uint8)
        self._rsp_off = self._grown(self._rsp_off, max_b + 1, torch.int64)
        ain = L.WireSeqAckIn(buf.data_ptr(), buf.numel(), off.data_ptr(), off.numel() - 1, self.n_dest, self.batch_id,
                             self.n_txn, 0, self.wait_client.data_ptr(), self.wait_startts.data_ptr(),
                             self.wait_acks.data_ptr())
        rout = L.WireRspOut(self._rsp_out.data_ptr(), cap, self._rsp_off.data_ptr(), max_b, 0)
        res = L.WireSeqAckResult(status=-1000)
        self.engine._after_torch()
        rc = L.lib().dv_wire_sequence_acks_device(self.engine._ctx, ctypes.byref(self.cfg), ctypes.byref(ain),
                                                  ctypes.byref(rout), ctypes.byref(res))
        _DeviceIngress._check(rc, res.status == rc, "dv_wire_sequence_acks_device")
        self._ack_held = (buf, off)
        if res.status != L.DV_OK:
            return self._rsp_out[:0], self._rsp_off[:0], 0, res
        return self._rsp_out[:res.n_bytes], self._rsp_off[:res.n_batches + 1], res.n_batches, res


def tpcc_gen_queries(p, n_txn, seed, home_part=0):
    """dv_tpcc_gen_queries: the client queries of dv_tpcc_gen (same draws)."""
    q = (L.TpccQuery * max(1, n_txn))()
    L.check(L.lib().dv_tpcc_gen_queries(ctypes.byref(p), seed, home_part, n_txn, q), "dv_tpcc_gen_queries")
    return q
