"""The TPC-C closed loop over decision lanes on the GPU
(dv_tpcc_epoch_run_closed_loop_lanes), plain, under a LoopTrack of 2 L buffers
and under a TpccLoopBackoff built over it (dv_tpcc_closed_loop_backoff_lanes),
against tests/test_tpcc_loop_lanes.py's reference -- LanesBackoffModel driven
by the oracle's TpccDB.epoch, never by the engine.  Integer work: everything
is compared bit for bit, with guard bytes behind every tracker and ring array.
Checked: every epoch's commit bytes, committed NewOrders' o_id and stats, the
cursor, each lane's next epoch (keys, types, tables, operation words, txn
ids), every column of every table, the tracker (log, epoch ends, histogram,
totals), the ring, the counters and all 2 L buffers' identity and abort
arrays.

Shapes (tests/test_tpcc_loop_lanes.py shows that they qualify): 512 txns are
two gather blocks, 1,000 four carry blocks with a ragged last; the closed form
commits one txn per epoch and parks the other 255.  6 L epochs visit every
(lane, buffer) pair three times.
"""
import ctypes

import numpy as np
import pytest

import _oracle as O
from test_loop_backoff import malformed_descs
from test_loop_backoff_lanes import MAX_LANES
from test_tpcc_loop_backoff import CCS, DB_SEED, ref_tpcc_backoff
from test_tpcc_loop_lanes import WIDE, WIDE_ACC, _closed_form_holds, host_tpcc_lanes_loop, ref_tpcc_lanes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import LoopBackoff, LoopTrack, TpccLoopBackoff  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc import tpcc as T  # noqa: E402
from test_loop_backoff_gpu import _check_ring as _check_ring_single  # noqa: E402
from test_loop_backoff_gpu import _check_track, _code, _guarded, _guards_stand  # noqa: E402
from test_loop_backoff_lanes_gpu import _check_ring, _untouched  # noqa: E402
from test_tpcc_closed_loop import MAX_TXN_ACC, _same_epoch  # noqa: E402
from test_tpcc_loop_backoff_gpu import _check_outcomes, _check_tables, _dev_pool, _host, _outputs  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


def _open(cc, pp, n, lanes, limits=None, max_txn=None, **eng_kw):
    eng = T.TpccEngine(cc, pp, max_txn or n, seed=DB_SEED, **eng_kw)
    extra = [eng.open_lane() for _ in range(lanes - 1)]
    if limits:
        for e in [eng] + extra:
            e.set_async_limits(*limits)
    return eng, extra


def _check_next(bufs, nxt, first, n):
    """every lane's next epoch (its first buffer) against the L epochs left"""
    out = []
    for ln, b in enumerate(bufs):
        e, e_args = b.epoch(0, n, MAX_TXN_ACC)
        _same_epoch(e, e_args, nxt[first + ln], f"lane {ln}: the epoch left in its buffers")
        out.append([t.cpu().numpy() for t in (e.keys, e.types, e.tables, e_args, e.acc_txn)])
    return out


def _run(cc, shape, D, lanes, slot_cap=None, limits=None, splits=None, ring=True, acc=MAX_TXN_ACC, queued=None,
         lane_timing=None, **eng_kw):
    """the shape's 6 L epochs (one call, or `splits` with resume) checked
    against the reference; D None: no tracker and no ring; ring False: the
    tracker alone (the reference at D = 1).  With slot_cap the model loses
    entries: the call fails with DV_ERR_ARG after its last epoch.  acc: the
    longest txn the pool declares (an epoch's bound is n_txn * acc).  queued:
    asserts how the epochs were decided, by their asynchronous launches --
    True: one each and none declined (queued ahead as round 0 plus the
    launch); False: none.  Returns what the D = 1 test compares."""
    kw = dict(slot_cap=slot_cap) if slot_cap else {}
    r = ref_tpcc_lanes(cc, shape, D or 1, lanes, **kw)
    pool, n, E, m = r["pool"], r["n"], r["epochs"], r["model"]
    splits = splits or (E,)
    assert sum(splits) == E
    eng, extra = _open(cc, r["pp"], n, lanes, limits, **eng_kw)
    try:
        if lane_timing:  # (on the last lane only)
            extra[-1].set_timing(lane_timing)
        trk = bo = held = None
        if D is not None:
            trk = LoopTrack(n, 2 * lanes, log_cap=n * E, epoch_cap=E)
            bo = TpccLoopBackoff(trk, D, slot_cap=slot_cap, lanes=lanes)
            held = _guarded(trk, bo)
            trk.attach(eng)
            if ring:
                bo.attach(eng)
        dpool, pargs, pb = _dev_pool(pool)
        dpool.max_txn_acc = acc
        cursor = torch.full((1,), r["cur0"], dtype=torch.int32, device="cuda")
        bufs = [T.TpccLoopBufs(n * acc, "cuda") for _ in range(lanes)]
        got, sts, done, yields = [], [], 0, 0
        for call, n_ep in enumerate(splits):
            commits, oids = _outputs(n, n_ep)

            def run():
                return eng.closed_loop_lanes(extra, dpool, pargs, pb, n, n_ep, cursor=cursor, bufs=bufs,
                                             d_commits=commits, d_oids=oids, resume=call > 0, track=trk)

            if m.lost and call == len(splits) - 1:
                assert _code(run) == L.DV_ERR_ARG
                sts = None
                trk.done += n_ep  # (the epochs ran and were logged: the error names the ring's capacity)
            else:
                s = run()[0]
                sts += s
                yields += sum(x.async_yields for x in s)
            torch.cuda.synchronize()
            got += _host(commits, oids)
            done += n_ep
            if len(splits) > 1:  # the state between two calls
                part = ref_tpcc_lanes(cc, shape, D or 1, lanes, epochs=done, **kw)
                assert int(cursor.item()) == part["model"].cur, call
                _check_next(bufs, part["nxt"], done, n)
                if bo is not None and ring:
                    _check_ring(trk, bo, part["model"], lanes, n)
        launched = declined = None
        if sts is not None:
            launched, declined = sum(x.async_launches for x in sts), sum(x.async_declined for x in sts)
            print("async launches / declined / yields:", launched, declined, yields)
        if limits:
            assert yields > 0, "no asynchronous launch yielded"
        if queued is not None:  # epochs queued ahead make one asynchronous launch each; one at a time, see the test
            assert (launched, declined) == ((E, 0) if queued else (0, 0)), (launched, declined)
        _check_outcomes(got, sts, r["ref"])
        assert int(cursor.item()) == m.cur
        nxt = _check_next(bufs, r["nxt"], E, n)
        _check_tables(eng, r["tables"])
        out = dict(commits=np.stack([c for c, _ in got]), oids=np.stack([o for _, o in got]),
                   cursor=int(cursor.item()), nxt=nxt)
        if trk is not None:
            _check_track(trk, m)
            if ring:
                _check_ring(trk, bo, m, lanes, n)
                assert bo.counters()[1] == m.lost
            else:
                assert sum(bo.counters()) == 0 and int(bo.slot_count.sum().item()) == 0
                assert int(torch.stack(bo.aborts).sum().item()) == 0
                for ln in range(lanes):
                    for b, k in ((2 * ln, m.k + ln), (2 * ln + 1, m.k - lanes + ln)):
                        assert np.array_equal(trk.ids[b][:n].cpu().numpy(), m.words(k)), f"ids of epoch {k}"
            _guards_stand(held)
            out.update(log=trk.log.cpu().numpy(), ends=trk.ends(), hist=trk.histogram(), totals=trk.totals(),
                       ids=[t[:n].cpu().numpy() for t in trk.ids])
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("lanes", [2, 3, 4])
def test_plain_loop(cc, lanes):
    """no tracker: 512 txns at 8 warehouses, 6 L epochs in one call, the pool
    wrapping in one of the first L takes"""
    _run(cc, "main", None, lanes)


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("lanes,D", [(2, 1), (2, 2), (2, 4), (2, 8), (3, 4), (3, 8), (4, 2), (4, 8)])
def test_tracker_and_ring(cc, lanes, D):
    _run(cc, "main", D, lanes)


def test_d1_equals_the_plain_tracked_lanes_loop():
    cc, lanes = dvcc.WAIT_DIE, 2
    got = _run(cc, "main", 1, lanes)
    plain = _run(cc, "main", 1, lanes, ring=False)
    assert sorted(got) == sorted(plain)
    for key in ("commits", "oids", "log", "ends", "hist"):
        assert np.array_equal(got[key], plain[key]), key
    assert got["cursor"] == plain["cursor"] and got["totals"] == plain["totals"]
    for b in range(2 * lanes):
        assert np.array_equal(got["ids"][b], plain["ids"][b]), f"ids of buffer {b}"
    for ln in range(lanes):
        for a, b in zip(got["nxt"][ln], plain["nxt"][ln]):
            assert np.array_equal(a, b), f"lane {ln}: the epoch left"


def test_one_lane_is_the_single_loop():
    """n_lanes == 1: dv_tpcc_epoch_run_closed_loop with dv_tpcc_closed_loop_backoff,
    against the single loop's reference and against that entry itself"""
    cc, D, E = dvcc.WAIT_DIE, 4, 6
    r = ref_tpcc_backoff(cc, "main", D, epochs=E)
    pool, n, m = r["pool"], r["n"], r["model"]
    res = []
    for lanes_entry in (True, False):
        eng = T.TpccEngine(cc, r["pp"], n, seed=DB_SEED)
        try:
            trk = LoopTrack(n, 2, log_cap=n * E, epoch_cap=E)
            bo = TpccLoopBackoff(trk, D)
            held = _guarded(trk, bo)
            trk.attach(eng)
            bo.attach(eng)
            dpool, pargs, pb = _dev_pool(pool)
            cursor = torch.full((1,), r["cur0"], dtype=torch.int32, device="cuda")
            commits, oids = _outputs(n, E)
            if lanes_entry:
                sts, bufs, cursor = eng.closed_loop_lanes([], dpool, pargs, pb, n, E, cursor=cursor, d_commits=commits,
                                                          d_oids=oids, track=trk)
                bufs = bufs[0]
            else:
                sts, bufs, cursor = eng.closed_loop(dpool, pargs, pb, n, E, cursor=cursor, d_commits=commits,
                                                    d_oids=oids, track=trk)
            torch.cuda.synchronize()
            got = _host(commits, oids)
            _check_outcomes(got, sts, r["ref"])
            assert int(cursor.item()) == m.cur
            e, e_args = bufs.epoch(0, n, MAX_TXN_ACC)
            _same_epoch(e, e_args, r["nxt"], "the epoch left in the buffers")
            _check_tables(eng, r["tables"])
            _check_track(trk, m)
            _check_ring_single(trk, bo, m, 0, n)
            _guards_stand(held)
            res.append([np.stack([c for c, _ in got]), np.stack([o for _, o in got]), trk.log.cpu().numpy(),
                        bo.park_ids.cpu().numpy(), bo.park_aborts.cpu().numpy(), e.keys.cpu().numpy(),
                        e_args.cpu().numpy()])
        finally:
            eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(*res))


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("lanes,D", [(2, 2), (2, 4), (4, 4)])
def test_closed_form(cc, lanes, D):
    """one warehouse, Payments only: every txn writes the warehouse row, so an
    epoch commits exactly its first txn whatever the CC"""
    r = ref_tpcc_lanes(cc, "closed form", D, lanes)
    assert _closed_form_holds(r)
    assert r["model"].spilled == {(2, 2): 256, (2, 4): 2256, (4, 4): 3051}[lanes, D]
    _run(cc, "closed form", D, lanes)


@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.OCC])
def test_forced_yields(cc):
    """asynchronous launches forced to yield on every lane: an epoch halts, the
    gate halts every epoch queued behind it, their refills are no-ops, and the
    host's redo logs, parks and builds each epoch once -- the results are the
    reference's"""
    assert ref_tpcc_lanes(cc, "main", 4, 2)["model"].spilled > 0
    _run(cc, "main", 4, 2, limits=(1, 1))


@pytest.mark.parametrize("eng_kw", [dict(asynchronous=False), dict(el64=True)])
def test_contexts_that_cannot_queue_ahead(eng_kw):
    """no asynchronous rounds, or 64-bit round elements: the decision follows
    its rounds from the host, so the epochs run one at a time, each with its
    refill -- the same results"""
    _run(dvcc.WAIT_DIE, "main", 4, 3, queued=False, **eng_kw)


@pytest.mark.parametrize("timing", [True, "kernel"])
def test_a_timing_flag_on_a_later_lane_only(timing):
    """the flag is looked for on every lane: with it on the last one alone no
    epoch is queued ahead of that lane's events -- the same results"""
    _run(dvcc.NO_WAIT, "main", 2, 3, lane_timing=timing)


def test_a_bound_past_the_small_epochs_limit():
    """16,400 txns declared at 128 accesses each: the bound, 2,099,200, is past
    the size up to which a decision is round 0 and one asynchronous launch on
    its own account, the epochs are a tenth of it; the loop queues that form
    all the same (a context sized like the benchmark's, 65,536 txns)"""
    r = ref_tpcc_lanes(dvcc.WAIT_DIE, WIDE, 4, 2)
    assert r["n"] * WIDE_ACC > 2 << 20 and r["model"].spilled > 0
    _run(dvcc.WAIT_DIE, WIDE, 4, 2, acc=WIDE_ACC, max_txn=65536, queued=True)


def test_two_calls_with_resume():
    """2 L and then 4 L epochs, the ring, the cursor and every lane's next
    epoch checked after each call"""
    _run(dvcc.WAIT_DIE, "main", 4, 2, splits=(4, 8))
    _run(dvcc.NO_WAIT, "main", 8, 3, splits=(6, 12))


def test_four_carry_blocks():
    """1,000 txns: four carry blocks, the last ragged; nothing lost at the
    default capacity"""
    m = ref_tpcc_lanes(dvcc.NO_WAIT, "four blocks", 4, 2)["model"]
    assert m.lost == 0 and m.spilled > 0
    _run(dvcc.NO_WAIT, "four blocks", 4, 2)


def test_capacity_exceeded():
    """1,100 entries a slot where the model wants more: 1,597 entries are
    counted and not written, the call says so after its last epoch, and the
    epochs, the log and the tables are still the model's"""
    m = ref_tpcc_lanes(dvcc.NO_WAIT, "four blocks", 4, 2, slot_cap=1100)["model"]
    assert (m.lost, m.fullest) == (1597, 1100)
    _run(dvcc.NO_WAIT, "four blocks", 4, 2, slot_cap=1100)


def _raw_desc(bo, n_entries, null_at=None):
    ptrs = [int(bo.aborts[i % len(bo.aborts)].data_ptr()) for i in range(n_entries)]
    if null_at is not None:
        ptrs[null_at] = None
    arr = (ctypes.c_void_p * n_entries)(*ptrs)
    return L.LoopBackoffDesc(bo.n_slots, bo.slot_cap, bo.park_ids.data_ptr(), bo.park_aborts.data_ptr(),
                             bo.slot_count.data_ptr(), arr, bo.ctr.data_ptr())


def _raw_loop(ctxs, dpool, pargs, pb, n, n_ep, cursor, bufs, buf_args="theirs"):
    """dv_tpcc_epoch_run_closed_loop_lanes itself over ctxs and bufs (one
    TpccLoopBufs per context); buf_args None: a NULL array of operation words"""
    nl = len(ctxs)
    arr = (L.EpochDev * (2 * nl))(*[b.desc(i) for b in bufs for i in range(2)])
    aps = None
    if buf_args is not None:
        aps = (ctypes.c_void_p * (2 * nl))(*[int(t.data_ptr()) for b in bufs for t in b.args])
    lp = (ctypes.c_void_p * nl)(*[e._ctx.value for e in ctxs])
    torch.cuda.synchronize()
    return L.lib().dv_tpcc_epoch_run_closed_loop_lanes(
        lp, nl, ctypes.byref(dpool.desc()), ctypes.c_void_p(pargs.data_ptr()), ctypes.c_void_p(pb.data_ptr()),
        ctypes.c_void_p(cursor.data_ptr()), n, arr, aps, bufs[0].cap, n_ep, 0, None, None, None)


def test_refusals():
    n = 256
    r = ref_tpcc_lanes(dvcc.NO_WAIT, "main", 2, 2)
    pp, pool = r["pp"], r["pool"]
    dpool, pargs, pb = _dev_pool(pool)
    cursor = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    f = L.lib().dv_tpcc_closed_loop_backoff_lanes
    loop = T.TpccEngine.closed_loop_lanes
    # ---- a context that is not DV_TPCC: at attach time and at the loop call
    ycsb = dvcc.CCEngine(dvcc.NO_WAIT, n, n * MAX_TXN_ACC)
    try:
        ycsb.load_ycsb_partition(1 << 10)
        ylane = ycsb.open_lane()
        trk = LoopTrack(n, 4, epoch_cap=8).attach(ycsb)
        bo = TpccLoopBackoff(trk, 2, lanes=2)
        assert _code(lambda: bo.attach(ycsb)) == L.DV_ERR_ARG
        assert bo.engine is None and getattr(ycsb, "_backoff", None) is None
        assert _code(lambda: loop(ycsb, [ylane], dpool, pargs, pb, n, 4, cursor=cursor, track=trk)) == L.DV_ERR_ARG
        _untouched(cursor, 77, [trk], [bo])
    finally:
        ycsb.close()
    # ---- CALVIN never aborts
    eng = T.TpccEngine(dvcc.CALVIN, pp, n, seed=DB_SEED)
    try:
        lane = eng.open_lane()
        bo = TpccLoopBackoff(LoopTrack(n, 4), 2, lanes=2)
        assert _code(lambda: bo.attach(eng)) == L.DV_ERR_STATE
        assert _code(lambda: loop(eng, [lane], dpool, pargs, pb, n, 4, cursor=cursor)) == L.DV_ERR_STATE
        _untouched(cursor, 77, [], [bo])
    finally:
        eng.close()
    eng, (lane1, lane2) = _open(dvcc.NO_WAIT, pp, n, 3)
    try:
        trk4 = LoopTrack(n, 4, epoch_cap=8)
        bo4 = TpccLoopBackoff(trk4, 2, lanes=2)
        # ---- at attach time
        assert _code(lambda: bo4.attach(eng)) == L.DV_ERR_STATE  # no tracker attached
        assert bo4.engine is None
        trk4.attach(eng)
        d4 = _raw_desc(bo4, 2 * (MAX_LANES + 1))
        assert f(eng._ctx, ctypes.byref(d4), 0) == L.DV_ERR_ARG
        assert f(eng._ctx, ctypes.byref(d4), MAX_LANES + 1) == L.DV_ERR_ARG
        assert f(eng._ctx, None, 0) == L.DV_ERR_ARG
        assert f(eng._ctx, ctypes.byref(d4), 3) == L.DV_ERR_STATE  # a tracker of four buffers, three lanes
        assert f(eng._ctx, ctypes.byref(d4), 1) == L.DV_ERR_STATE
        assert f(eng._ctx, ctypes.byref(_raw_desc(bo4, 4, null_at=3)), 2) == L.DV_ERR_ARG
        for name, d in malformed_descs():
            assert f(eng._ctx, ctypes.byref(d), 2) == L.DV_ERR_ARG, name
        assert _code(lambda: TpccLoopBackoff(trk4, 3, lanes=2).attach(eng)) == L.DV_ERR_ARG
        with pytest.raises(ValueError):
            TpccLoopBackoff(trk4, 2)  # (a lanes tracker under the single loop's ring)
        with pytest.raises(ValueError):
            bo4.swap()
        # ---- at the loop call: arguments (nothing is attached but trk4)
        def call(lanes, trk, n_ep=4, args=pargs, bufs=None):
            return _code(lambda: eng.closed_loop_lanes(lanes, dpool, args, pb, n, n_ep, cursor=cursor, bufs=bufs,
                                                       track=trk))

        assert call([lane1], trk4, args=None) == L.DV_ERR_ARG  # no operation words of the pool
        holed = [T.TpccLoopBufs(n * MAX_TXN_ACC, "cuda") for _ in range(2)]
        holed[1].args[1] = None
        assert call([lane1], trk4, bufs=holed) == L.DV_ERR_ARG  # a buffer without operation words
        whole = [T.TpccLoopBufs(n * MAX_TXN_ACC, "cuda") for _ in range(2)]
        assert _raw_loop([eng, lane1], dpool, pargs, pb, n, 4, cursor, whole, buf_args=None) == L.DV_ERR_ARG
        _untouched(cursor, 77, [trk4], [bo4])
        assert call([lane1], trk4, n_ep=9) == L.DV_ERR_ARG  # a tracker without room for the epochs
        trk2 = LoopTrack(n, 2, epoch_cap=8).attach(eng)
        eng._track = None  # (past the Python check: the context holds a tracker of two buffers)
        assert call([lane1], None) == L.DV_ERR_ARG
        _untouched(cursor, 77, [trk2, trk4], [bo4])
        # ---- a ring attached through another entry, under the tracker the lanes loop needs
        bo_y1, bo_y2, bo_t1 = LoopBackoff(trk2, 2), LoopBackoff(trk4, 2), TpccLoopBackoff(trk2, 2)
        for bo, trk in ((bo_y1, trk2), (bo_y2, trk4), (bo_t1, trk2)):
            trk.attach(eng)
            bo.attach(eng)
            trk4.attach(eng)  # (the back-off stays attached)
            assert call([lane1], trk4) == L.DV_ERR_STATE
            bo.detach()
        _untouched(cursor, 77, [trk2, trk4], [bo_y1, bo_y2, bo_t1, bo4])
        # ---- attached for two lanes: a call over three, and the single loop
        trk4.attach(eng)
        bo4.attach(eng)
        trk6 = LoopTrack(n, 6, epoch_cap=8).attach(eng)
        assert call([lane1, lane2], trk6, n_ep=6) == L.DV_ERR_STATE
        trk2.attach(eng)
        assert _code(lambda: eng.closed_loop(dpool, pargs, pb, n, 2, cursor=cursor, track=trk2)) == L.DV_ERR_STATE
        _untouched(cursor, 77, [trk2, trk4, trk6], [bo4])
        # ---- a back-off on a lane that is not the first
        trk4.attach(eng)
        bo4.detach()
        t1 = LoopTrack(n, 4, epoch_cap=8).attach(lane1)
        b1 = TpccLoopBackoff(t1, 2, lanes=2).attach(lane1)
        assert call([lane1], trk4) == L.DV_ERR_STATE
        _untouched(cursor, 77, [trk4, t1], [bo4, b1])
        t1.detach()
        assert b1.engine is None
        # detaching through the new entry, then the tracker with the ring
        bo4.attach(eng)
        bo4.detach()
        assert bo4.engine is None and eng._backoff is None
        bo4.attach(eng)
        trk4.detach()
        assert bo4.engine is None
        # ---- a lane inside an epoch (closed with its owner, unfinished)
        one = T.gen(pp, 8, 3)
        dep, d_args = T.device_epoch(one)
        lane2.begin_tpcc(dep, d_args)
        assert call([lane1, lane2], None, n_ep=6) == L.DV_ERR_STATE
        assert int(cursor.item()) == 77
    finally:
        eng.close()


@pytest.mark.parametrize("where", ["lanes[0]", "a later lane"])
def test_refuses_a_communicator(where):
    """a communicator (the in-process transport, one rank) on the first lane,
    or on a later lane only: DV_ERR_STATE before any launch, with the cursor,
    the tracker and the ring -- attached before the communicator was made --
    untouched; without it the same call is accepted by the same checks"""
    n = 256
    r = ref_tpcc_lanes(dvcc.NO_WAIT, "main", 2, 2)
    dpool, pargs, pb = _dev_pool(r["pool"])
    cursor = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    eng, (lane1,) = _open(dvcc.NO_WAIT, r["pp"], n, 2)
    try:
        trk = LoopTrack(n, 4, epoch_cap=8).attach(eng)
        bo = TpccLoopBackoff(trk, 2, lanes=2).attach(eng)
        dvcc.CCEngine.comm_init_local([eng if where == "lanes[0]" else lane1])
        assert _code(lambda: eng.closed_loop_lanes([lane1], dpool, pargs, pb, n, 4, cursor=cursor, track=trk)) \
            == L.DV_ERR_STATE
        bufs = [T.TpccLoopBufs(n * MAX_TXN_ACC, "cuda") for _ in range(2)]
        assert _raw_loop([eng, lane1], dpool, pargs, pb, n, 4, cursor, bufs) == L.DV_ERR_STATE
        _untouched(cursor, 77, [trk], [bo])
        assert int(torch.stack(bo.aborts).sum().item()) == 0 and int(torch.stack(trk.ids).sum().item()) == 0
    finally:
        eng.close()


def test_replies_end_to_end():
    """client batches ingested on the device are the loop's pool; over two
    lanes under D = 4 every epoch's slice of the commit log -- retried and
    released txns among them -- is answered byte for byte as
    tests/wire_fmt.py encodes it"""
    import test_wire_device_tpcc_cases as C
    import wire_fmt as W
    from dvcc.wire import TpccDeviceWireIngress, WireIngress, tpcc_gen_queries
    from test_wire_device_tpcc import _query_messages, _reply_batches
    cc, POOL, N, E, D, lanes = dvcc.WAIT_DIE, 1000, 300, 8, 4, 2
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
    ref, nxt, m, tables = host_tpcc_lanes_loop(cc, po, pool, 0, N, E, D, lanes)
    assert m.totals[3] >= 1 and m.spilled > 0, "no released txn commits / nothing spills"
    eng, extra = _open(cc, pp, N, lanes)
    try:
        ing = TpccDeviceWireIngress(eng, pp, POOL, POOL * 33)
        dep, taken, status = ing.feed_buffer(buf, off)
        assert (taken, status, dep.n_txn, dep.n_acc) == (len(batches), L.DV_OK, POOL, pool.n_acc)
        trk = LoopTrack(N, 2 * lanes, log_cap=N * E, epoch_cap=E)
        bo = TpccLoopBackoff(trk, D, lanes=lanes)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        commits, oids = _outputs(N, E)
        sts, bufs, cursor = eng.closed_loop_lanes(extra, dep, dep.args, dep.txn_begin, N, E, d_commits=commits,
                                                  d_oids=oids, track=trk)
        torch.cuda.synchronize()
        _check_outcomes(_host(commits, oids), sts, ref)
        _check_tables(eng, tables)
        _check_track(trk, m)
        _check_ring(trk, bo, m, lanes, N)
        for k in range(E):
            src = m.log[k][0]
            assert ing.respond_logged(trk.commits(k)[0]) == _reply_batches(
                0, pool.txn_id[src], pool.client_startts[src], pool.return_node[src]), f"epoch {k}: replies"
        _guards_stand(held)
    finally:
        eng.close()
