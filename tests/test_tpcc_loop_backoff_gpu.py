"""Back-off in the TPC-C closed loop on the GPU (dv_tpcc_closed_loop_backoff):
dv_tpcc_epoch_run_closed_loop under a LoopTrack and a TpccLoopBackoff against
tests/test_tpcc_loop_backoff.py's reference -- BackoffModel driven by the
oracle's TpccDB.epoch, never by the engine.  Integer work: everything is
compared bit for bit, with guard bytes behind every tracker and ring array.
Checked: every epoch's commit bytes, committed NewOrders' o_id and stats, the
cursor, the epoch left in the buffers (keys, types, tables, operation words,
txn ids), every column of every table, the tracker (log, epoch ends,
histogram, totals), the ring, the counters and both buffers' identity and
abort arrays.

Shapes (tests/test_tpcc_loop_backoff.py, which also shows that they qualify):
512 txns are two gather blocks, 1,000 four carry blocks with a ragged last;
the closed form commits one txn per epoch and parks the other 255.
"""
import ctypes

import numpy as np
import pytest

import _oracle as O
from test_loop_backoff_gpu import _check_ring, _check_track, _code, _guarded, _guards_stand
from test_tpcc_closed_loop import MAX_TXN_ACC, _same_epoch, _same_outcome
from test_tpcc_loop_backoff import CCS, DB_SEED, host_tpcc_backoff_loop, ref_tpcc_backoff

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import LoopBackoff, LoopTrack, TpccLoopBackoff  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc import tpcc as T  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


def _dev_pool(pool):
    dpool, pargs = T.device_epoch(pool)
    assert dpool.max_txn_acc <= MAX_TXN_ACC
    dpool.max_txn_acc = MAX_TXN_ACC
    return dpool, pargs, torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()


def _outputs(n, n_ep):
    return ([torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(n_ep)],
            [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(n_ep)])


def _host(commits, oids):
    return [(c.cpu().numpy().copy(), o.cpu().numpy().view(np.uint64).copy()) for c, o in zip(commits, oids)]


def _check_outcomes(got, sts, ref):
    """commit bytes and o_id of every epoch; sts (None: the call failed after
    its last epoch and returned none): the stats"""
    assert len(got) == len(ref)
    for k, ((c, o), (c_ref, o_ref, st_ref, host)) in enumerate(zip(got, ref)):
        if sts is not None:
            _same_outcome(k, c, o, sts[k], c_ref, o_ref, st_ref, host)
        assert np.array_equal(c[:host.n_txn], c_ref) and np.array_equal(o[:host.n_txn], o_ref), k


def _check_tables(eng, tables):
    for t in range(5):
        for col in range(3):
            assert (eng.read_col(t, col) == tables[t][1 + col]).all(), f"table {t} col {col}"


def _check_next(bufs, nxt, n):
    e, e_args = bufs.epoch(0, n, MAX_TXN_ACC)
    _same_epoch(e, e_args, nxt, "the epoch left in the buffers")
    return e, e_args


def _run(cc, shape, D, slot_cap=None):
    """one call of the shape's epochs (an even count) checked against the
    reference; returns what the D = 1 test compares.  With slot_cap the model
    loses entries: the call fails with DV_ERR_ARG after its last epoch."""
    r = ref_tpcc_backoff(cc, shape, D, **(dict(slot_cap=slot_cap) if slot_cap else {}))
    pool, n, E, m = r["pool"], r["n"], r["epochs"], r["model"]
    eng = T.TpccEngine(cc, r["pp"], n, seed=DB_SEED)
    try:
        trk = LoopTrack(n, 2, log_cap=n * E, epoch_cap=E)
        bo = TpccLoopBackoff(trk, D, slot_cap=slot_cap)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pargs, pb = _dev_pool(pool)
        cursor = torch.full((1,), r["cur0"], dtype=torch.int32, device="cuda")
        bufs = T.TpccLoopBufs(n * MAX_TXN_ACC, "cuda")
        commits, oids = _outputs(n, E)

        def call():
            return eng.closed_loop(dpool, pargs, pb, n, E, cursor=cursor, bufs=bufs, d_commits=commits, d_oids=oids,
                                   track=trk)

        if m.lost:
            assert _code(call) == L.DV_ERR_ARG
            sts = None
            trk.done += E  # (the epochs ran and were logged: the error names the ring's capacity)
        else:
            sts = call()[0]
        torch.cuda.synchronize()
        got = _host(commits, oids)
        _check_outcomes(got, sts, r["ref"])
        assert int(cursor.item()) == m.cur
        e, e_args = _check_next(bufs, r["nxt"], n)
        _check_tables(eng, r["tables"])
        _check_track(trk, m)
        _check_ring(trk, bo, m, 0, n)
        assert bo.counters()[1] == m.lost
        _guards_stand(held)
        return dict(commits=np.stack([c for c, _ in got]), oids=np.stack([o for _, o in got]),
                    cursor=int(cursor.item()), log=trk.log.cpu().numpy(), ends=trk.ends(), hist=trk.histogram(),
                    totals=trk.totals(), ids=[t[:n].cpu().numpy() for t in trk.ids],
                    nxt=[t.cpu().numpy() for t in (e.keys, e.types, e.tables, e_args, e.acc_txn)])
    finally:
        eng.close()


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("D", [1, 2, 4, 8])
def test_main_shape(cc, D):
    """512 txns at 8 warehouses, 24 epochs in one call, the pool wrapping in
    the first take and in a later refill"""
    _run(cc, "main", D)


def test_main_shape_longest_delay_16():
    """all five delay classes: a txn's fifth abort parks it 16 epochs ahead"""
    assert ref_tpcc_backoff(dvcc.NO_WAIT, "main", 16)["most"] >= 5
    _run(dvcc.NO_WAIT, "main", 16)


def test_d1_equals_the_plain_tracked_loop():
    cc = dvcc.WAIT_DIE
    got = _run(cc, "main", 1)
    r = ref_tpcc_backoff(cc, "main", 1)
    pool, n, E = r["pool"], r["n"], r["epochs"]
    eng = T.TpccEngine(cc, r["pp"], n, seed=DB_SEED)
    try:
        trk = LoopTrack(n, 2, log_cap=n * E, epoch_cap=E).attach(eng)
        dpool, pargs, pb = _dev_pool(pool)
        cursor = torch.full((1,), r["cur0"], dtype=torch.int32, device="cuda")
        commits, oids = _outputs(n, E)
        sts, bufs, cursor = eng.closed_loop(dpool, pargs, pb, n, E, cursor=cursor, d_commits=commits, d_oids=oids,
                                            track=trk)
        torch.cuda.synchronize()
        assert np.array_equal(torch.stack(commits).cpu().numpy(), got["commits"])
        assert np.array_equal(torch.stack(oids).cpu().numpy().view(np.uint64), got["oids"])
        assert int(cursor.item()) == got["cursor"]
        assert np.array_equal(trk.log.cpu().numpy(), got["log"]) and list(trk.ends()) == list(got["ends"])
        assert np.array_equal(trk.histogram(), got["hist"]) and trk.totals() == got["totals"]
        for b in range(2):
            assert np.array_equal(trk.ids[b][:n].cpu().numpy(), got["ids"][b])
        e, e_args = bufs.epoch(0, n, MAX_TXN_ACC)
        for a, b in zip((e.keys, e.types, e.tables, e_args, e.acc_txn), got["nxt"]):
            assert np.array_equal(a.cpu().numpy(), b)
    finally:
        eng.close()


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("D", [2, 8])
def test_closed_form(cc, D):
    """one warehouse, Payments only: every txn writes the warehouse row, so an
    epoch commits exactly its first txn whatever the CC"""
    r = ref_tpcc_backoff(cc, "closed form", D)
    assert all(int(c.sum()) == 1 and c[0] == 1 for c, _, _, _ in r["ref"])
    assert r["model"].spilled == {2: 258, 8: 1483}[D]
    _run(cc, "closed form", D)


@pytest.mark.parametrize("limits", [None, (1, 1)])
def test_calls_swaps_and_reattach(limits):
    """12 epochs as calls of 3, 5 and 4 with resume: the three swaps after the
    odd calls, the ring checked after every call, and before the last call a
    drained log with tracker and ring attached again at epoch 8.  With
    asynchronous launches forced to yield, a halted epoch is decided again
    synchronously before its refill is queued: parked and built once."""
    cc, D, splits = dvcc.WAIT_DIE, 4, (3, 5, 4)
    total = sum(splits)
    final = ref_tpcc_backoff(cc, "main", D, epochs=total)
    pool, n, fm = final["pool"], final["n"], final["model"]
    assert fm.spilled > 0
    eng = T.TpccEngine(cc, final["pp"], n, seed=DB_SEED)
    try:
        if limits:
            eng.set_async_limits(*limits)
        trk = LoopTrack(n, 2, log_cap=n * total, epoch_cap=8)
        bo = TpccLoopBackoff(trk, D)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pargs, pb = _dev_pool(pool)
        cursor = torch.full((1,), final["cur0"], dtype=torch.int32, device="cuda")
        bufs = T.TpccLoopBufs(n * MAX_TXN_ACC, "cuda")
        got, sts, done, yields = [], [], 0, 0
        for call, n_ep in enumerate(splits):
            if call == len(splits) - 1:
                trk.drain()
                trk.attach(eng, first_epoch=done)
                bo.detach()
                bo.attach(eng)
            commits, oids = _outputs(n, n_ep)
            s, bufs, cursor = eng.closed_loop(dpool, pargs, pb, n, n_ep, cursor=cursor, bufs=bufs, d_commits=commits,
                                              d_oids=oids, resume=call > 0, track=trk)
            got += _host(commits, oids)
            sts += s
            yields += sum(x.async_yields for x in s)
            done += n_ep
            if n_ep & 1:
                bufs.swap()
                trk.swap()
                bo.swap()
            m = ref_tpcc_backoff(cc, "main", D, epochs=done)
            assert int(cursor.item()) == m["model"].cur, call
            _check_ring(trk, bo, m["model"], 0, n)
            _check_next(bufs, m["nxt"], n)
        if limits:
            assert yields > 0, "no asynchronous launch yielded"
        _check_outcomes(got, sts, final["ref"])
        _check_tables(eng, final["tables"])
        # the tracker since the second attach: the last call's log
        first = total - splits[-1]
        assert list(trk.ends()) == [e - fm.epoch_end[first - 1] for e in fm.epoch_end[first:]]
        for i in range(splits[-1]):
            src, born = trk.commits(i)
            assert np.array_equal(src.cpu().numpy(), fm.log[first + i][0]), i
            assert np.array_equal(born.cpu().numpy(), fm.log[first + i][1]), i
        assert np.array_equal(trk.histogram(), fm.hist) and trk.totals() == fm.totals
        _guards_stand(held)
    finally:
        eng.close()


def test_four_carry_blocks():
    """1,000 txns: four carry blocks, the last ragged; nothing lost at the
    default capacity"""
    assert ref_tpcc_backoff(dvcc.NO_WAIT, "four blocks", 4)["model"].lost == 0
    _run(dvcc.NO_WAIT, "four blocks", 4)


def test_capacity_exceeded():
    """1,100 entries a slot where the model wants more: 3,720 entries are
    counted and not written, the call says so after its last epoch, and the
    epochs, the log and the tables are still the model's"""
    assert ref_tpcc_backoff(dvcc.NO_WAIT, "four blocks", 4, slot_cap=1100)["model"].lost == 3720
    _run(dvcc.NO_WAIT, "four blocks", 4, slot_cap=1100)


def _raw_attach(eng, bo):
    """dv_tpcc_closed_loop_backoff over bo's arrays, whatever their number"""
    arr = (ctypes.c_void_p * len(bo.aborts))(*[int(t.data_ptr()) for t in bo.aborts])
    d = L.LoopBackoffDesc(bo.n_slots, bo.slot_cap, bo.park_ids.data_ptr(), bo.park_aborts.data_ptr(),
                          bo.slot_count.data_ptr(), arr, bo.ctr.data_ptr())
    return L.lib().dv_tpcc_closed_loop_backoff(eng._ctx, ctypes.byref(d))


def _untouched(bo, trk=None):
    torch.cuda.synchronize()
    assert sum(bo.counters()) == 0 and int(bo.slot_count.sum().item()) == 0
    assert int(bo.park_ids.abs().sum().item()) == 0 and int(bo.park_aborts.sum().item()) == 0
    if trk is not None:
        assert int(trk.tot.sum().item()) == 0 and int(trk.log_pos.item()) == 0


def test_refusals():
    n = 256
    pp = ref_tpcc_backoff(dvcc.NO_WAIT, "main", 2)["pp"]
    ycsb = dvcc.CCEngine(dvcc.NO_WAIT, n, n * 10)
    try:
        ycsb.load_ycsb_partition(1 << 10)
        trk = LoopTrack(n, 2, epoch_cap=4).attach(ycsb)
        bo = TpccLoopBackoff(trk, 2)
        assert _code(lambda: bo.attach(ycsb)) == L.DV_ERR_ARG  # a YCSB context
        assert bo.engine is None and getattr(ycsb, "_backoff", None) is None
        _untouched(bo, trk)
    finally:
        ycsb.close()
    eng = T.TpccEngine(dvcc.CALVIN, pp, n, seed=DB_SEED)
    try:
        bo = TpccLoopBackoff(LoopTrack(n, 2), 2)
        assert _code(lambda: bo.attach(eng)) == L.DV_ERR_STATE  # CALVIN never aborts
        _untouched(bo)
    finally:
        eng.close()
    eng = T.TpccEngine(dvcc.NO_WAIT, pp, n, seed=DB_SEED)
    try:
        trk = LoopTrack(n, 2, epoch_cap=4)
        bo = TpccLoopBackoff(trk, 2)
        assert _code(lambda: bo.attach(eng)) == L.DV_ERR_STATE  # no tracker attached
        trk.attach(eng)
        assert _code(lambda: TpccLoopBackoff(trk, 3).attach(eng)) == L.DV_ERR_ARG
        trk.detach()
        trk4 = LoopTrack(n, 4, epoch_cap=4).attach(eng)
        bo4 = LoopBackoff(trk4, 2)
        assert _raw_attach(eng, bo4) == L.DV_ERR_STATE  # a tracker of four buffers
        with pytest.raises(ValueError):
            TpccLoopBackoff(trk4, 2)
        _untouched(bo)
        _untouched(bo4, trk4)
    finally:
        eng.close()


@pytest.mark.parametrize("how", ["ring detached", "tracker detached"])
def test_a_detached_ring_leaves_the_plain_loop(how):
    """attached and then detached -- itself, or its tracker -- the ring is not
    touched and the loop is the plain one (the reference at D = 1)"""
    cc, E = dvcc.OCC, 6
    r = ref_tpcc_backoff(cc, "main", 1, epochs=E)
    pool, n, m = r["pool"], r["n"], r["model"]
    eng = T.TpccEngine(cc, r["pp"], n, seed=DB_SEED)
    try:
        trk = LoopTrack(n, 2, log_cap=n * E, epoch_cap=E).attach(eng)
        bo = TpccLoopBackoff(trk, 4).attach(eng)
        bo.detach()
        bo.attach(eng)
        if how == "ring detached":
            bo.detach()
        else:
            trk.detach()  # (and the back-off with it)
        assert bo.engine is None
        dpool, pargs, pb = _dev_pool(pool)
        cursor = torch.full((1,), r["cur0"], dtype=torch.int32, device="cuda")
        commits, oids = _outputs(n, E)
        sts, bufs, cursor = eng.closed_loop(dpool, pargs, pb, n, E, cursor=cursor, d_commits=commits, d_oids=oids)
        torch.cuda.synchronize()
        _check_outcomes(_host(commits, oids), sts, r["ref"])
        assert int(cursor.item()) == m.cur
        _check_next(bufs, r["nxt"], n)
        _check_tables(eng, r["tables"])
        if how == "ring detached":
            _check_track(trk, m)
        _untouched(bo, trk if how == "tracker detached" else None)
        assert int(torch.stack(bo.aborts).sum().item()) == 0
    finally:
        eng.close()


def test_replies_end_to_end():
    """client batches ingested on the device are the loop's pool; under D = 4
    every epoch's slice of the commit log -- retried and released txns among
    them -- is answered byte for byte as tests/wire_fmt.py encodes it"""
    import test_wire_device_tpcc_cases as C
    import wire_fmt as W
    from dvcc.wire import TpccDeviceWireIngress, WireIngress, tpcc_gen_queries
    from test_wire_device_tpcc import _query_messages, _reply_batches
    cc, POOL, N, E, D = dvcc.WAIT_DIE, 1000, 300, 6, 4
    kw = dict(num_wh=4, cust_per_dist=1000, max_items=2000)
    pp, po = T.tpcc_params(**kw), O.tpcc_params(**kw)
    qs = tpcc_gen_queries(pp, POOL, 910)
    clients = [W.batches(0, 1 + k, _query_messages(qs, POOL, 5000)[k::2]) for k in range(2)]
    batches = [b for pair in zip(*clients) for b in pair] + clients[0][len(clients[1]):] + clients[1][len(clients[0]):]
    buf, off = C.stream(batches)
    host = WireIngress(L.TPCC, POOL, POOL * 33, tpcc=pp)
    assert host.feed_buffer(buf, off) == []
    pool = host.take()
    assert pool.n_txn == POOL and len(set(pool.return_node.tolist())) == 2
    ref, nxt, m, tables, _ = host_tpcc_backoff_loop(cc, po, pool, 0, N, E, D)
    assert m.totals[3] >= 1 and m.spilled > 0, "no released txn commits / nothing spills"
    eng = T.TpccEngine(cc, pp, N, seed=DB_SEED)
    try:
        ing = TpccDeviceWireIngress(eng, pp, POOL, POOL * 33)
        dep, taken, status = ing.feed_buffer(buf, off)
        assert (taken, status, dep.n_txn, dep.n_acc) == (len(batches), L.DV_OK, POOL, pool.n_acc)
        trk = LoopTrack(N, 2, log_cap=N * E, epoch_cap=E)
        bo = TpccLoopBackoff(trk, D)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        commits, oids = _outputs(N, E)
        sts, bufs, cursor = eng.closed_loop(dep, dep.args, dep.txn_begin, N, E, d_commits=commits, d_oids=oids,
                                            track=trk)
        torch.cuda.synchronize()
        _check_outcomes(_host(commits, oids), sts, ref)
        _check_track(trk, m)
        _check_ring(trk, bo, m, 0, N)
        for k in range(E):
            src = m.log[k][0]
            assert ing.respond_logged(trk.commits(k)[0]) == _reply_batches(
                0, pool.txn_id[src], pool.client_startts[src], pool.return_node[src]), f"epoch {k}: replies"
        _guards_stand(held)
    finally:
        eng.close()
