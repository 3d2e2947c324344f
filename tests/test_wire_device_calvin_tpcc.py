"""dv_wire_ingest_device_calvin_tpcc on the GPU against the host decoder
(dv_wire_open / dv_wire_decode_batches through WireIngress under a calvin = 1,
DV_TPCC cfg) and the oracle -- never against the device path itself.  Where a
call stops comes from the model of tests/test_wire_device_calvin_tpcc_cases.py
(checked there against the host decoder), the arrays from the host decoder run
with ample capacity over exactly the taken messages.

The kernels' tiles (dvcc_wire_layout.h): W = 4 mbufs per workgroup of
k_wire_check_calvin_tpcc / k_wire_emit_calvin_tpcc (kWireWave), S = 3,072 mbufs
per scan chunk (kWireChunk).  The decode tests run on a YCSB context: the entry
takes the stream and its per-call words from the context, the access lists
from cfg->tpcc.
"""
import ctypes

import numpy as np
import pytest

import _oracle as O
import wire_fmt as W
import test_wire_device_calvin_tpcc_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc import tpcc as T  # noqa: E402
from dvcc.wire import CalvinTpccDeviceWireIngress, WireEpoch, WireIngress, tpcc_gen_queries  # noqa: E402

WAVE, CHUNK = 4, 3072
GUARD = 0xA5
PAD = 64  # guard elements behind every output's capacity
U64 = C.U64
E0 = 9  # the batch id of the case builders
PER_TXN = {"txn_type": torch.uint8, "txn_id": torch.int64, "client_startts": torch.int64, "return_node": torch.int32}
PER_ACC = {"keys": torch.int64, "types": torch.uint8, "acc_txn": torch.int32, "tables": torch.uint8,
           "args": torch.int64, "owner": torch.uint8}
PRIOR = (5, 17, 1, 3)  # an epoch so far: txns, accesses, RDONEs, longest txn


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    e = dvcc.CCEngine(dvcc.CALVIN, 8192, 1 << 17)
    yield e
    e.close()


class Outputs:
    """device output buffers of max_txn / max_acc, every byte GUARD, PAD more
    elements behind each"""

    def __init__(self, max_txn, max_acc, optional=True):
        g = lambda n, dt: torch.full((n * torch.empty(0, dtype=dt).element_size(),), GUARD, dtype=torch.uint8,  # noqa
                                     device="cuda").view(dt)
        T_, A = max_txn + PAD, max(1, max_acc) + PAD
        self.max_txn, self.max_acc = max_txn, max_acc
        self.t = dict(txn_begin=g(T_ + 1, torch.int32))
        self.t.update({k: g(A, dt) for k, dt in PER_ACC.items() if optional or k != "owner"})
        if optional:
            self.t.update(n_acc_dev=g(1 + PAD, torch.int32))
            self.t.update({k: g(T_, dt) for k, dt in PER_TXN.items()})

    def struct(self):
        p = lambda k: self.t[k].data_ptr() if k in self.t else None  # noqa: E731
        return L.WireTpccDevOut(self.max_txn, 0, self.max_acc, p("txn_begin"), p("n_acc_dev"), p("keys"), p("types"),
                                p("acc_txn"), p("tables"), p("args"), p("txn_type"), p("owner"), p("txn_id"),
                                p("client_startts"), p("return_node"))

    def host(self):
        torch.cuda.synchronize()  # (the outputs are written on the engine's stream)
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def upload(buf, off, shift=0):
    """the stream `shift` bytes into its tensor"""
    t = torch.zeros(shift + len(buf) + 16, dtype=torch.uint8, device="cuda")
    t[shift:shift + len(buf)] = torch.from_numpy(buf)
    return t[shift:], torch.from_numpy(off.view(np.int64)).cuda()


def status_of(stop, n_txn):
    if stop == C.END:
        return L.DV_OK
    if stop in (C.MALFORMED, C.STALE) or (stop == C.CAPACITY and n_txn == 0):
        return L.DV_ERR_ARG
    return L.WIRE_MORE


def check_arrays(h, ref, t0, a0):
    """the call's outputs behind txn t0 / access a0 equal the host decoder's
    epoch `ref`, bit for bit; the guards in front of the append point and
    behind the new totals stand"""
    n, a = t0 + ref.n_txn, a0 + ref.n_acc
    u = lambda x, dt: x.view(dt)  # noqa: E731
    assert (u(h["txn_begin"], np.uint32)[t0:n + 1] == a0 + ref.txn_begin.astype(np.int64)).all()
    for k, dt in (("keys", np.uint64), ("args", np.uint64)):
        d = np.flatnonzero(u(h[k], dt)[a0:a] != getattr(ref, k))
        assert d.size == 0, f"{k} at {d[:5]}: {u(h[k], dt)[a0:a][d[:5]]} for {getattr(ref, k)[d[:5]]}"
    assert (h["types"][a0:a] == ref.types).all()
    assert (h["tables"][a0:a] == ref.tables).all()
    assert (u(h["acc_txn"], np.uint32)[a0:a] == t0 + ref.acc_txn().astype(np.int64)).all()
    if "owner" in h:
        assert u(h["n_acc_dev"], np.uint32)[0] == a
        assert (h["owner"][a0:a] == ref.owner).all()
        assert (h["txn_type"][t0:n] == ref.txn_type).all()
        assert (u(h["txn_id"], np.uint64)[t0:n] == ref.txn_id).all()  # (the message's own, the sequencer's)
        assert (u(h["client_startts"], np.uint64)[t0:n] == ref.client_startts).all()
        assert (u(h["return_node"], np.uint32)[t0:n] == ref.return_node).all()
    for k, v in h.items():
        lo = 0 if k == "n_acc_dev" else t0 if k in PER_TXN or k == "txn_begin" else a0
        hi = n + 1 if k == "txn_begin" else 1 if k == "n_acc_dev" else n if k in PER_TXN else a
        assert (v[:lo].view(np.uint8) == GUARD).all(), f"{k}: written in front of {lo}"
        assert (v[hi:].view(np.uint8) == GUARD).all(), f"{k}: written past {hi}"


def run_and_check(eng, mbufs, cur=(0, 0), E=None, prior=(0, 0, 0, 0), max_txn=4096, max_acc=1 << 16, shift=0,
                  bad=(), off=None, buf_len=None, optional=True, expect=None, pset="base"):
    """One call (again after a window's end) over `mbufs` from the cursor into
    guarded buffers, appended behind `prior` = (txns, accesses, rdones, longest
    txn) of an epoch so far; everything compared with the model and the host
    decoder.  expect: (stop, cursor) the case must come to.  Returns pos."""
    buf, off0 = C.stream(mbufs)
    off = off0 if off is None else off
    t0, a0, r0, m0 = prior
    stop, at, e_out, taken, t, a, r, mx = C.model(mbufs, set(bad), cur, E, t0, a0, max_txn, max_acc)
    if expect is not None:
        assert (stop, at) == expect
    d_buf, d_off = upload(buf, off, shift)
    outs = Outputs(max_txn, max_acc, optional)
    pos = L.WireCalvinPos(cur[0], cur[1], t0, r0, a0, U64 if E is None else E, m0, 77)
    cfg, out = C.wire_cfg(pset), outs.struct()
    eng._after_torch()
    while True:
        before = (pos.batch, pos.n_txn)
        rc = L.lib().dv_wire_ingest_device_calvin_tpcc(eng._ctx, ctypes.byref(cfg), d_buf.data_ptr(),
                                                       len(buf) if buf_len is None else buf_len, d_off.data_ptr(),
                                                       len(mbufs), ctypes.byref(out), ctypes.byref(pos))
        if pos.stop != C.WINDOW:
            break
        # a window is max(max_txn - n_txn + 1, 256) mbufs
        assert rc == L.WIRE_MORE and pos.msg == 0 and pos.batch - before[0] == max(max_txn - before[1] + 1, 256)
    assert (pos.stop, (pos.batch, pos.msg)) == (stop, at)
    ref = C.host_decode(C.repack(mbufs, taken), pset)
    assert (ref.n_txn, ref.n_acc, ref.rdone) == (t, a, r)
    assert (pos.n_txn, pos.n_acc, pos.rdone) == (t0 + t, a0 + a, r0 + r)
    assert pos.batch_id == (U64 if e_out is None else e_out)
    assert pos.max_txn_acc == max(m0, ref.max_txn_acc() if t else 0) == max(m0, mx)
    assert rc == status_of(stop, pos.n_txn)
    check_arrays(outs.host(), ref, t0, a0)
    return pos


def _q(rng, bid, n=0, cst=0, tid=0, pset="base"):
    """a Payment (n = 0) or a NewOrder of n items"""
    p = C.PSETS[pset]
    if n:
        x = C.neworder(C._items(rng, n, p, 1), 1 + n % p.num_wh)
    else:
        x = C.pay(1 + tid % p.num_wh, 1 + cst % 10, 1 + tid % 1000)
    return C.tmsg(x, bid, cst, tid, rng)


def _good_row(rng, n, bid=E0):
    return [C.mbuf([_q(rng, bid, i % 3, 10 * i, 3 * i)], 5 + i % 2) for i in range(n)]


# ---- message shapes
@pytest.mark.parametrize("pset", list(C.PSETS))
@pytest.mark.parametrize("prior", [(0, 0, 0, 0), PRIOR], ids=["fresh_epoch", "appended"])
def test_every_message_shape_in_one_stream(eng, prior, pset):
    cases = C.good_cases(pset)
    mbufs = [c[1] for c in cases]
    assert max(len(b) for b in mbufs) == 4096 and any(len(b) == 4044 for b in mbufs)
    pos = run_and_check(eng, mbufs, prior=prior, expect=(C.END, (len(mbufs), 0)), pset=pset)
    assert pos.n_txn - prior[0] == sum(c[2] for c in cases) and pos.n_acc - prior[1] == sum(c[3] for c in cases)
    assert pos.rdone - prior[2] == sum(c[4] for c in cases) and pos.max_txn_acc == 127 and pos.batch_id == E0
    run_and_check(eng, mbufs, prior=prior, optional=False, pset=pset)


@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_any_byte_alignment_of_the_buffer(eng, shift):
    run_and_check(eng, [c[1] for c in C.good_cases()], shift=shift, prior=(3, 4, 0, 2))
    name, mbufs, cur, E = C.cut_cases()[1]
    run_and_check(eng, mbufs, cur, E, shift=shift)


# ---- the cut
@pytest.mark.parametrize("case", C.cut_cases(), ids=lambda c: c[0])
def test_the_stream_is_cut_where_the_batch_id_changes(eng, case):
    name, mbufs, cur, E = case
    pos = run_and_check(eng, mbufs, cur, E, prior=(2, 9, 0, 6))
    if pos.stop == C.BATCH:  # resuming at the cursor: the next batch's epoch, as the host decoder cuts it
        nxt = run_and_check(eng, mbufs, (pos.batch, pos.msg), None)
        assert nxt.batch_id > (E if pos.batch_id == U64 else pos.batch_id) and nxt.n_txn + nxt.rdone > 0


@pytest.mark.parametrize("cut", [False, True], ids=["to_the_end", "cut_in_the_last"])
@pytest.mark.parametrize("n", [1, WAVE - 1, WAVE, WAVE + 1, CHUNK, CHUNK + 1])
def test_mbuf_counts_around_the_kernels_tiles(eng, n, cut):
    rng = np.random.default_rng(n)
    one = [C.mbuf([_q(rng, E0, 0, i, 2 * i)], 5 + i % 3) for i in range(8)] + [C.mbuf([C.rdone(E0, rng)], 6)]
    mbufs = [one[i % 9] for i in range(n)]  # (one-Payment or RDONE-only mbufs)
    if cut:
        mbufs[-1] = C.mbuf([_q(rng, E0, 3, 1, 1), C.rdone(E0, rng), _q(rng, E0 + 1, 2, 2, 2)], 5)
    run_and_check(eng, mbufs, max_txn=CHUNK + 8, max_acc=4 * CHUNK,
                  expect=(C.BATCH, (n - 1, 2)) if cut else (C.END, (n, 0)))


def test_rdone_only_mbufs_past_the_window_are_taken_by_calling_again(eng):
    rng = np.random.default_rng(4)
    mbufs = [C.mbuf([C.rdone(E0, rng)], 5) for _ in range(700)] + [C.mbuf([_q(rng, E0, 2), C.rdone(E0, rng)], 6)]
    pos = run_and_check(eng, mbufs, max_txn=4, max_acc=16, expect=(C.END, (701, 0)))
    assert (pos.n_txn, pos.rdone) == (1, 701)
    ing = CalvinTpccDeviceWireIngress(eng, C.PSETS["base"], 4, 16, node_id=C.NODE, node_cnt=C.NODE_CNT,
                                      part_cnt=C.PART_CNT)
    p = ing.feed_buffer(*C.stream(mbufs))
    assert (p.stop, p.batch, p.msg, p.rdone, ing.status) == (C.END, 701, 0, 701, L.DV_OK)
    ep = ing.take()
    assert (ep.n_txn, ep.n_acc, ep.rdone, ep.batch_id, ep.max_txn_acc) == (1, 7, 701, E0, 7)
    assert ep.tables.numel() == ep.args.numel() == ep.owner.numel() == 7 and ep.txn_type.tolist() == [2]


# ---- capacity
def _capacity_stream():
    """26 mbufs of 1, 2, 3, 1, ... queries (Payments and NewOrders of up to 5
    items), an RDONE-only mbuf among them, and their running counts"""
    rng = np.random.default_rng(21)
    mbufs, txns, accs = [], [], []
    for i in range(26):
        items = [(2 * i + 3 * j + 1) % 6 for j in range(1 + i % 3)] if i != 6 else []
        msgs = [_q(rng, E0, n, 100 * i + j, 7 * i + j) for j, n in enumerate(items)] or [C.rdone(E0, rng)]
        mbufs.append(C.mbuf(msgs, src=5 + i % 2))
        txns.append(len(items))
        accs.append(sum(3 + 2 * n for n in items))
    return mbufs, np.cumsum(txns), np.cumsum(accs)


@pytest.mark.parametrize("kind", ["txn_at_mbuf_end", "txn_one_short", "acc_cuts_first"])
def test_capacity_cuts_at_whole_mbufs_and_continues(eng, kind):
    mbufs, ct, ca = _capacity_stream()
    if kind == "txn_at_mbuf_end":
        max_txn, max_acc = int(ct[9]), 1 << 12
    elif kind == "txn_one_short":
        assert ct[10] - ct[9] >= 2
        max_txn, max_acc = int(ct[10]) - 1, 1 << 12
    else:
        max_txn, max_acc = int(ct[20]), int(ca[7]) + 1
        assert ca[8] - ca[7] >= 2
    cur, n_epochs, total = (0, 0), 0, 0
    while True:
        pos = run_and_check(eng, mbufs, cur, E0, max_txn=max_txn, max_acc=max_acc)
        assert pos.stop in (C.CAPACITY, C.END) and pos.n_txn > 0
        if n_epochs == 0:
            want = {"txn_at_mbuf_end": (10, int(ct[9])), "txn_one_short": (10, int(ct[9])),
                    "acc_cuts_first": (8, int(ct[7]))}[kind]
            assert (pos.batch, pos.n_txn) == want and pos.msg == 0
        cur, n_epochs, total = (pos.batch, pos.msg), n_epochs + 1, total + pos.n_txn
        if pos.stop == C.END:
            break
    assert n_epochs >= 2 and total == ct[-1]


def test_a_127_access_neworder_straddling_max_acc(eng):
    rng = np.random.default_rng(24)
    mbufs = _good_row(rng, 3) + [C.mbuf([_q(rng, E0, 62, 1, 1)], 5), C.mbuf([_q(rng, E0, 0, 2, 2)], 5)]
    a3 = 3 + 5 + 7
    for room, expect in ((a3 + 126, (C.CAPACITY, (3, 0))), (a3 + 127, (C.CAPACITY, (4, 0))),
                         (a3 + 130, (C.END, (5, 0)))):
        pos = run_and_check(eng, mbufs, max_acc=room, expect=expect)
        assert pos.max_txn_acc == (127 if expect[1][0] > 3 else 7)
    # the same behind an epoch so far: the room is what the earlier calls left
    run_and_check(eng, mbufs, E=E0, prior=PRIOR, max_acc=PRIOR[1] + a3 + 126, expect=(C.CAPACITY, (3, 0)))


def test_capacity_comes_before_the_batch_cut_of_the_same_mbuf(eng):
    rng = np.random.default_rng(22)
    mbufs = _good_row(rng, 3) + [C.mbuf([_q(rng, E0), _q(rng, E0, 2), C.rdone(E0, rng), _q(rng, E0 + 1)], 5)]
    run_and_check(eng, mbufs, max_txn=4, expect=(C.CAPACITY, (3, 0)))
    run_and_check(eng, mbufs, max_txn=5, expect=(C.BATCH, (3, 3)))
    # ... but an empty run never fails it: the mbuf of the later batch stops a full epoch as BATCH
    mbufs = _good_row(rng, 3) + [C.mbuf([_q(rng, E0 + 1), _q(rng, E0 + 1, 62)], 5)]
    run_and_check(eng, mbufs, max_txn=3, max_acc=15, expect=(C.BATCH, (3, 0)))


def test_a_first_mbuf_that_can_never_fit_and_rdones_at_full_capacity(eng):
    rng = np.random.default_rng(23)
    two = C.mbuf([_q(rng, E0, 0), _q(rng, E0, 1)], 5)  # 3 + 5 accesses
    pos = run_and_check(eng, [two], max_txn=1, expect=(C.CAPACITY, (0, 0)))
    assert pos.n_txn == 0 and pos.batch_id == U64  # (DV_ERR_ARG: status_of)
    run_and_check(eng, [two], max_acc=7, expect=(C.CAPACITY, (0, 0)))
    # the same mbuf behind a txn of the epoch: DV_WIRE_MORE
    run_and_check(eng, [two], E=E0, prior=(1, 3, 0, 3), max_txn=2, expect=(C.CAPACITY, (0, 0)))
    # an epoch at max_txn still takes RDONEs, and stops at the next query
    full = (8, 24, 0, 5)
    run_and_check(eng, [C.mbuf([C.rdone(E0, rng)], 5)], E=E0, prior=full, max_txn=8, max_acc=24,
                  expect=(C.END, (1, 0)))
    run_and_check(eng, [C.mbuf([C.rdone(E0, rng), C.rdone(E0, rng)], 5), two], E=E0, prior=full, max_txn=8,
                  max_acc=24, expect=(C.CAPACITY, (1, 0)))


# ---- malformed
@pytest.mark.parametrize("kind", C.malformed_kinds(), ids=lambda k: k[0])
def test_a_malformed_message_stops_the_call_at_its_mbuf(eng, kind):
    """the bad message first, in the middle and last in its mbuf, that mbuf
    first, in the middle and last in the stream; then outside the run, in
    front of the cursor and behind the cut"""
    rng = np.random.default_rng(5)
    row = _good_row(rng, 9)
    for where, k in ((0, 0), (2, 4), (4, 8), (0, 8), (4, 0)):
        mbufs = list(row)
        mbufs[k] = C.malformed_mbuf(kind, where)
        run_and_check(eng, mbufs, bad=[k], prior=PRIOR, expect=(C.MALFORMED, (k, 0)))
    front, behind = C.outside_run_mbufs(kind)
    run_and_check(eng, [front] + row[:2], cur=(0, 1), bad=[0], prior=PRIOR, expect=(C.MALFORMED, (0, 1)))
    run_and_check(eng, row[:4] + [behind] + row[4:6], bad=[4], prior=PRIOR, expect=(C.MALFORMED, (4, 0)))


@pytest.mark.parametrize("case", C.batch_level_cases(), ids=lambda c: c[0])
def test_a_malformed_mbuf_stops_the_call_at_it(eng, case):
    rng = np.random.default_rng(5)
    for k in (0, 4, 8):
        mbufs = _good_row(rng, 9)
        mbufs[k] = case[1]
        run_and_check(eng, mbufs, bad=[k], prior=PRIOR, expect=(C.MALFORMED, (k, 0)))


@pytest.mark.parametrize("case", C.OFF_CASES)
def test_a_bad_offset_stops_the_call_at_its_mbuf(eng, case):
    rng = np.random.default_rng(6)
    for k in (0, 4, 8):
        mbufs = _good_row(rng, 9)
        buf, off = C.stream(mbufs)
        if case == "off_decreases":
            if k:
                off[k + 1] = int(off[k]) - 1
            else:  # (mbuf 0 starts at 0: it starts at 1 and ends at 0 instead)
                off[0], off[1] = 1, 0
        else:
            off[k + 1:] = len(buf) + 8
        run_and_check(eng, mbufs, bad=[k], off=off, prior=PRIOR, expect=(C.MALFORMED, (k, 0)))
    # an end inside the allocation but past buf_len
    mbufs = _good_row(rng, 3)
    run_and_check(eng, mbufs, bad=[2], buf_len=len(C.stream(mbufs)[0]) - 1, expect=(C.MALFORMED, (2, 0)))


def test_a_cursor_at_the_message_count_is_malformed(eng):
    rng = np.random.default_rng(7)
    mbufs = [C.mbuf([_q(rng, E0), _q(rng, E0, 2)], 5)] + _good_row(rng, 2)
    run_and_check(eng, mbufs, cur=(0, 2), prior=PRIOR, expect=(C.MALFORMED, (0, 2)))
    run_and_check(eng, mbufs, cur=(0, 64), prior=PRIOR, expect=(C.MALFORMED, (0, 64)))
    run_and_check(eng, mbufs, cur=(0, 1), expect=(C.END, (3, 0)))


def test_a_malformed_mbuf_behind_another_stopper_is_not_reported(eng):
    rng = np.random.default_rng(8)
    badm = C.malformed_mbuf(dict((k[0], k) for k in C.malformed_kinds())["item_ol_i_id_0"], 2)
    mbufs = _good_row(rng, 3) + [C.mbuf([C.rdone(E0, rng), _q(rng, E0 + 1)], 5), _good_row(rng, 1, E0 + 1)[0], badm]
    pos = run_and_check(eng, mbufs, bad=[5], expect=(C.BATCH, (3, 1)))
    # ... and the next batch's call reaches it
    run_and_check(eng, mbufs, (pos.batch, pos.msg), None, bad=[5], expect=(C.MALFORMED, (5, 0)))
    # behind a capacity stop
    mbufs = _good_row(rng, 3) + [badm]
    run_and_check(eng, mbufs, bad=[3], max_txn=2, expect=(C.CAPACITY, (2, 0)))


# ---- arguments
def test_refused_arguments_touch_nothing(eng):
    rng = np.random.default_rng(9)
    d_buf, d_off = upload(*C.stream(_good_row(rng, 3)))
    for name, cfg, out, pos in C.refused_arguments():
        before = bytes(pos)
        assert C.ingest(eng._ctx, cfg, out, pos, d_buf.data_ptr(), d_off.data_ptr()) == L.DV_ERR_ARG, name
        assert bytes(pos) == before, name
    outs = Outputs(16, 160)
    pos = C._pos(batch=4)
    assert C.ingest(eng._ctx, C.wire_cfg(), outs.struct(), pos, d_buf.data_ptr(), d_off.data_ptr()) == L.DV_ERR_ARG
    assert all((v.view(np.uint8) == GUARD).all() for v in outs.host().values())
    # the TPC-C client entry goes on refusing CALVIN on a live context
    r, o, cfg = L.WireDevResult(status=77), outs.struct(), C.wire_cfg()
    assert L.lib().dv_wire_ingest_device_tpcc(eng._ctx, ctypes.byref(cfg), d_buf.data_ptr(), 64, d_off.data_ptr(), 3,
                                              0, ctypes.byref(o), 0, ctypes.byref(r)) == L.DV_ERR_ARG
    assert r.status == 77 and all((v.view(np.uint8) == GUARD).all() for v in outs.host().values())


# ---- several sequencers, one epoch
def _concat(parts):
    """dvcc.sequence of host-decoded TPC-C epochs, with what it does not carry"""
    ref = dvcc.sequence(parts)
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])  # noqa: E731
    return WireEpoch(ref.keys, ref.types, ref.txn_begin, cat("tables"), args=cat("args"), txn_type=cat("txn_type"),
                     owner=cat("owner"), txn_id=cat("txn_id"), client_startts=cat("client_startts"),
                     return_node=cat("return_node"))


def _equal(dep, ref):
    torch.cuda.synchronize()
    u = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    assert (u(dep.keys, np.uint64) == ref.keys).all() and (u(dep.types, np.uint8) == ref.types).all()
    assert (u(dep.tables, np.uint8) == ref.tables).all() and (u(dep.args, np.uint64) == ref.args).all()
    assert (u(dep.owner, np.uint8) == ref.owner).all() and (u(dep.txn_type, np.uint8) == ref.txn_type).all()
    assert (u(dep.acc_txn, np.uint32) == ref.acc_txn()).all()
    assert (u(dep.txn_begin, np.uint32) == ref.txn_begin).all()
    assert (u(dep.txn_id, np.uint64) == ref.txn_id).all()
    assert (u(dep.client_startts, np.uint64) == ref.client_startts).all()
    assert (u(dep.return_node, np.uint32) == ref.return_node).all()


def test_streams_appended_in_node_order_equal_the_sequenced_host_epochs(eng):
    rng = np.random.default_rng(10)
    tid = iter(range(1, 10_000))
    q = lambda bid, n: _q(rng, bid, n, 1000 + n, next(tid))  # noqa: E731
    s0 = [C.mbuf([q(E0, 3), q(E0, 0), q(E0, 7)], 10), C.mbuf([q(E0, 2), C.rdone(E0, rng), q(E0 + 1, 4)], 10)]
    s1 = [C.mbuf([q(E0 - 1, 2), C.rdone(E0 - 1, rng), q(E0, 5)], 11),
          C.mbuf([q(E0, 1), q(E0, 62), C.rdone(E0, rng), q(E0 + 1, 1)], 11)]
    s2 = [C.mbuf([q(E0 + 1, 2)], 12)]  # (this sequencer's batch E0 never came: nothing taken)
    ing = CalvinTpccDeviceWireIngress(eng, C.PSETS["base"], 64, 512, node_id=C.NODE, node_cnt=C.NODE_CNT,
                                      part_cnt=C.PART_CNT)
    dep, cursors = ing.sequence([C.stream(s) for s in (s0, s1, s2)], [None, (0, 2), None])
    assert cursors == [(1, 2), (1, 3), (0, 0)]
    parts = [C.host_decode(C.repack(s0, [(0, 0, 3), (1, 0, 2)])), C.host_decode(C.repack(s1, [(0, 2, 3), (1, 0, 3)]))]
    ref = _concat(parts)
    assert (dep.n_txn, dep.n_acc, dep.rdone, dep.batch_id, dep.max_txn_acc) == (ref.n_txn, ref.n_acc, 2, E0, 127)
    _equal(dep, ref)
    with pytest.raises(L.DvccError):  # a stale message (the second stream's first) is no end of a batch
        ing.sequence([C.stream(s1), C.stream(s1)], [(0, 2), (0, 0)])


# ---- end to end
def _query_messages(qs, n, bid, ids):
    """tpcc_gen_queries' queries as a sequencer's forwarded CL_QRY messages of batch bid"""
    msgs = []
    for i in range(n):
        x = qs[i]
        msgs.append(W.tpcc_query(dict(
            txn_type=x.txn_type, w_id=x.w_id, d_id=x.d_id, c_id=x.c_id, d_w_id=x.d_w_id, c_w_id=x.c_w_id,
            c_d_id=x.c_d_id, c_last=bytes(x.c_last), h_amount=x.h_amount, by_last_name=x.by_last_name,
            ol_cnt=x.ol_cnt, o_entry_d=x.o_entry_d, parts=[x.parts[k] for k in range(x.n_parts)],
            items=[(x.items[k].ol_i_id, x.items[k].ol_supply_w_id, x.items[k].ol_quantity)
                   for k in range(x.ol_cnt)]), client_startts=int(ids[i]) * 3, txn_id=int(ids[i]), batch_id=bid))
    return msgs


def test_two_sequencers_tpcc_streams_through_the_engine():
    """Two sequencers' continuous streams of two Calvin batches (ids 4 and 5,
    300 queries each per batch, batch 5 starting inside an mbuf): each epoch
    sequenced on the device, run by a CALVIN TpccEngine and compared with the
    oracle's TpccDB over the host-decoded epochs in node order -- commit
    bytes, o_ids and final tables; every txn acknowledged as the host packer
    does.  Every txn of both batches commits (CALVIN aborts none), so none is
    left out of the comparison."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    n, kw = 300, dict(num_wh=4, cust_per_dist=1000, max_items=2000)
    pp, po = T.tpcc_params(**kw), O.tpcc_params(**kw)
    streams, host = [], []
    for node in range(2):
        msgs = []
        for k, bid in enumerate((4, 5)):
            ids = node + 2 * (k * n + np.arange(n))
            msgs += _query_messages(tpcc_gen_queries(pp, n, 70 + 2 * node + k), n, bid, ids) + [W.rdone(bid)]
        mbufs = W.batches(0, 10 + node, msgs)
        kinds = [{x[3] for x in C.parse_mbuf(b)} for b in mbufs]
        assert {4, 5} in kinds  # batch 5 starts mid-mbuf
        streams.append(C.stream(mbufs))
        w = WireIngress(L.TPCC, n, 33 * n, node_id=0, node_cnt=2, calvin=True, tpcc=pp)
        closed = []
        for b in mbufs:
            closed += w.feed(b)
        closed.append(w.take())
        assert [(d.n_txn, d.rdone, d.batch_id) for d in closed] == [(n, 1, 4), (n, 1, 5)]
        host.append((w, closed))
    db = O.TpccDB(po, 5)
    eng = T.TpccEngine(dvcc.CALVIN, pp, 2 * n, seed=5)
    try:
        ing = CalvinTpccDeviceWireIngress(eng, pp, 2 * n, 66 * n, node_id=0, node_cnt=2)
        d_streams = [upload(buf, off) for buf, off in streams]
        cursors = None
        for k, bid in enumerate((4, 5)):
            dep, cursors = ing.sequence(d_streams, cursors)
            ref = _concat([host[node][1][k] for node in range(2)])
            ref.batch_id = bid
            assert (dep.n_txn, dep.n_acc, dep.rdone, dep.batch_id) == (2 * n, ref.n_acc, 2, bid)
            _equal(dep, ref)
            c_ref, o_ref, st_ref = db.epoch(O.CALVIN, ref.keys, ref.types, ref.tables, ref.args, ref.txn_begin)
            assert c_ref.all() and st_ref.committed == 2 * n  # the condition: every txn commits, on the oracle first
            d_commit = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
            d_oid = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
            st = eng.run_tpcc_epoch_device(dep, dep.args, d_commit, d_oid)
            assert (d_commit.cpu().numpy() == c_ref).all() and st.committed == 2 * n
            assert (d_oid.cpu().numpy().view(np.uint64) == o_ref).all()
            acks = ing.respond(dep)
            assert acks == host[0][0].respond(ref)
            assert sum(len(W.parse_batch(b, calvin=True)[2]) for b in acks) == 2 * n
        assert [c[0] for c in cursors] == [len(s[1]) - 1 for s in streams] and all(c[1] == 0 for c in cursors)
        for t in range(5):
            tab = db.table(t)
            for col in range(3):
                assert (eng.read_col(t, col) == tab[1 + col]).all(), f"table {t} col {col}"
    finally:
        eng.close()
