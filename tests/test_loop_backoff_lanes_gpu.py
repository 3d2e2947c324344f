"""Back-off in the closed loop over decision lanes on the GPU
(dv_closed_loop_backoff_lanes): the lanes loop run under a dvcc.LoopTrack of
2 L buffers and a dvcc.LoopBackoff built over it, against
tests/test_loop_backoff_lanes.py's numpy model, driven by the oracle's commit
bytes -- never by the engine's.  Checked: every epoch's commit bytes and
stats, the cursor, the table, each lane's next epoch, the identity and abort
arrays of all 2 L buffers, every slot's contents and count, the tracker's log,
epoch ends, histogram and totals, the four counters, and the guard bytes
behind every array.

Shapes: 2,000 txns are seven full carry blocks of 256 and a ragged one (8,192
rows), 6 L epochs; the closed form (300 txns, one write of key 1 each, one
commit per epoch) parks 299 txns per epoch.  A test that relies on spill, on
a delay class or on lost entries asserts that on the model first.
"""
import ctypes

import numpy as np
import pytest

from test_carry import host_closed_loop_lanes
from test_loop_backoff import CF_N, CF_POOL, ROWS, malformed_descs
from test_loop_backoff_lanes import E16, MAX_LANES, N, POOL_KEY, ref_backoff_lanes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import _oracle as O  # noqa: E402
import dvcc  # noqa: E402
from dvcc import LoopBackoff, LoopTrack  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from test_loop_backoff_gpu import (_check_next, _check_outcomes, _check_track, _code, _dev_pool, _engine,  # noqa: E402
                                   _guarded, _guards_stand)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


def _check_ring(trk, bo, model, lanes, n_txn):
    """the ring, the counters and all 2 L buffers' identity and abort arrays,
    after a multiple of 2 L epochs: lane l's first buffer holds epoch
    model.k + l (built, undecided), its second epoch model.k - L + l"""
    torch.cuda.synchronize()
    assert model.k % (2 * lanes) == 0
    cnt = bo.slot_count.cpu().numpy().view(np.uint32)
    assert list(cnt) == [len(s[0]) for s in model.slots]
    for s, ((src, born, ab), (msrc, mborn, mab)) in enumerate(zip(bo.parked(), model.slots)):
        assert np.array_equal(src, msrc) and np.array_equal(born, mborn), f"slot {s}"
        assert np.array_equal(ab, mab.astype(np.uint8)), f"slot {s}: aborts"
    assert bo.counters() == model.counters()
    for ln in range(lanes):
        for b, k in ((2 * ln, model.k + ln), (2 * ln + 1, model.k - lanes + ln)):
            assert np.array_equal(trk.ids[b][:n_txn].cpu().numpy(), model.words(k)), f"ids of epoch {k}"
            assert np.array_equal(bo.aborts[b][:n_txn].cpu().numpy(), model.aborts_of(k)), f"aborts of epoch {k}"


def _open(cc, lanes, n_txn, acc, prefix, rows, async_iters=None):
    eng = _engine(cc, n_txn, acc, prefix, rows)
    extra = [eng.open_lane() for _ in range(lanes - 1)]
    if async_iters:
        for e in [eng] + extra:
            e.set_async_limits(async_iters, 0)
    return eng, extra


def _run(cc, D, lanes, prefix, pool_key=POOL_KEY, n_txn=N, n_epochs=None, rows=ROWS, acc=10, n_bins=64):
    """one call of n_epochs (a multiple of 2 L) epochs; returns what the D = 1 test compares"""
    n_epochs = n_epochs if n_epochs is not None else 6 * lanes
    kw = dict(n_bins=n_bins) if n_bins != 64 else {}
    pool, ref, nxt, model, f0 = ref_backoff_lanes(cc, pool_key, n_txn, n_epochs, D, lanes, rows=rows, **kw)
    eng, extra = _open(cc, lanes, n_txn, acc, prefix, rows)
    try:
        trk = LoopTrack(n_txn, 2 * lanes, log_cap=n_txn * n_epochs, epoch_cap=n_epochs, n_bins=n_bins)
        bo = LoopBackoff(trk, D)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(n_txn, dtype=torch.uint8, device="cuda") for _ in range(n_epochs)]
        sts, bufs, cursor = eng.closed_loop_lanes(extra, dpool, pb, n_txn, n_epochs, d_commits=commits, track=trk)
        got = [(c.cpu().numpy(), s) for c, s in zip(commits, sts)]
        _check_outcomes(got, ref)
        assert int(cursor.item()) == model.cur
        for ln in range(lanes):
            _check_next(bufs[ln], 0, nxt[n_epochs + ln], n_txn, pool)
        assert np.array_equal(eng.read_table(0, rows), f0)
        _check_track(trk, model)
        _check_ring(trk, bo, model, lanes, n_txn)
        _guards_stand(held)
        nx = [bufs[ln].epoch(0, n_txn, acc) for ln in range(lanes)]
        return dict(commits=np.stack([c for c, _ in got]), cursor=int(cursor.item()), log=trk.log.cpu().numpy(),
                    ends=trk.ends(), hist=trk.histogram(), totals=trk.totals(),
                    ids=[t[:n_txn].cpu().numpy() for t in trk.ids], keys=[e.keys.cpu().numpy() for e in nx],
                    acc_txn=[e.acc_txn.cpu().numpy() for e in nx], types=[e.types.cpu().numpy() for e in nx])
    finally:
        eng.close()


def _assert_model(cc, D, lanes, n_epochs=None):
    model = ref_backoff_lanes(cc, POOL_KEY, N, n_epochs if n_epochs is not None else 6 * lanes, D, lanes)[3]
    if D > 1:
        assert model.spilled > 0 and model.classes >= set(range(min(model.lgD, 3) + 1))
    assert model.totals[3] >= 1 and model.lost == 0
    return model


@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC])
@pytest.mark.parametrize("D", [1, 2, 4, 8])
@pytest.mark.parametrize("prefix", [400, None])
def test_two_lanes(cc, D, prefix):
    """2,000 txns on 8,192 rows, 12 epochs over two lanes: the pipelined
    tb-form loop (prefix 400) and epochs one at a time in the keys form
    (prefix off)"""
    _assert_model(cc, D, 2)
    _run(cc, D, 2, prefix)


@pytest.mark.parametrize("cc,D,lanes,prefix", [(dvcc.NO_WAIT, 4, 3, 400), (dvcc.OCC, 8, 3, None),
                                               (dvcc.WAIT_DIE, 2, 3, 400), (dvcc.NO_WAIT, 8, 4, 400),
                                               (dvcc.WAIT_DIE, 4, 4, None), (dvcc.OCC, 2, 4, 400)])
def test_three_and_four_lanes(cc, D, lanes, prefix):
    """three lanes: a lane count that is not a power of two against a ring that is"""
    _assert_model(cc, D, lanes)
    _run(cc, D, lanes, prefix)


@pytest.mark.parametrize("lanes", [2, 4])
def test_longest_delay_16(lanes):
    """all five delay classes: a txn's fifth abort parks it L - 1 + 16 epochs ahead"""
    model = _assert_model(dvcc.NO_WAIT, 16, lanes, E16[lanes])
    assert model.classes == {0, 1, 2, 3, 4}
    _run(dvcc.NO_WAIT, 16, lanes, 400, n_epochs=E16[lanes])


@pytest.mark.parametrize("lanes,prefix", [(2, 400), (3, None)])
def test_d1_equals_the_plain_tracked_lanes_loop(lanes, prefix):
    cc, E = dvcc.NO_WAIT, 6 * lanes
    got = _run(cc, 1, lanes, prefix)
    pool = ref_backoff_lanes(cc, POOL_KEY, N, E, 1, lanes)[0]
    eng, extra = _open(cc, lanes, N, 10, prefix, ROWS)
    try:
        trk = LoopTrack(N, 2 * lanes, log_cap=N * E, epoch_cap=E, n_bins=64).attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop_lanes(extra, dpool, pb, N, E, d_commits=commits, track=trk)
        torch.cuda.synchronize()
        assert np.array_equal(torch.stack(commits).cpu().numpy(), got["commits"])
        assert int(cursor.item()) == got["cursor"]
        assert np.array_equal(trk.log.cpu().numpy(), got["log"]) and list(trk.ends()) == list(got["ends"])
        assert np.array_equal(trk.histogram(), got["hist"]) and trk.totals() == got["totals"]
        for b in range(2 * lanes):
            assert np.array_equal(trk.ids[b][:N].cpu().numpy(), got["ids"][b])
        for ln in range(lanes):
            e = bufs[ln].epoch(0, N, 10)
            assert np.array_equal(e.keys.cpu().numpy(), got["keys"][ln])
            assert np.array_equal(e.types.cpu().numpy(), got["types"][ln])
            assert np.array_equal(e.acc_txn.cpu().numpy(), got["acc_txn"][ln])
    finally:
        eng.close()


@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("D", [2, 8])
def test_closed_form(D, lanes):
    model = ref_backoff_lanes(dvcc.NO_WAIT, "closed form", CF_N, 40, D, lanes, rows=16, n_bins=8)[3]
    assert model.spilled > 0 and model.cur == sum(len(d) for d in model.drawn) % CF_POOL
    _run(dvcc.NO_WAIT, D, lanes, None, "closed form", CF_N, 40, rows=16, acc=1, n_bins=8)


def test_forced_yields_and_resume():
    """asynchronous launches forced to yield on every lane (an epoch halts, the
    gate halts every epoch queued behind it, their refills are no-ops, and the
    host's redo parks and builds each epoch once), a first call and two resume
    calls of 2 L epochs, the ring checked after each"""
    cc, lanes, D, calls = dvcc.NO_WAIT, 2, 4, 3
    per = 2 * lanes
    total = calls * per
    pool, ref, nxt, final, f0 = ref_backoff_lanes(cc, POOL_KEY, N, total, D, lanes)
    assert final.spilled > 0
    eng, extra = _open(cc, lanes, N, 10, 400, ROWS, async_iters=1)
    try:
        trk = LoopTrack(N, 2 * lanes, log_cap=N * total, epoch_cap=total)
        bo = LoopBackoff(trk, D)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(per)]
        cursor, bufs, got, yields = None, None, [], 0
        for call in range(calls):
            sts, bufs, cursor = eng.closed_loop_lanes(extra, dpool, pb, N, per, cursor=cursor, bufs=bufs,
                                                      d_commits=commits, resume=call > 0, track=trk)
            got += [(c.cpu().numpy().copy(), s) for c, s in zip(commits, sts)]
            yields += sum(s.async_yields for s in sts)
            # the model after the same epochs (its own run: the cached one is read-only)
            m = ref_backoff_lanes(cc, POOL_KEY, N, (call + 1) * per, D, lanes)[3]
            _check_ring(trk, bo, m, lanes, N)
            assert int(cursor.item()) == m.cur, call
        assert yields > 0, "no asynchronous launch yielded"
        _check_outcomes(got, ref)
        for ln in range(lanes):
            _check_next(bufs[ln], 0, nxt[total + ln], N, pool)
        assert np.array_equal(eng.read_table(0, ROWS), f0)
        _check_track(trk, final)
        _guards_stand(held)
    finally:
        eng.close()


def test_capacity_exceeded():
    """closed form, two lanes, D = 2, 300 entries a slot where the model reaches 597"""
    cc, lanes, n_ep, cap = dvcc.NO_WAIT, 2, 40, 300
    assert ref_backoff_lanes(cc, "closed form", CF_N, n_ep, 2, lanes, rows=16)[3].fullest > cap
    pool, ref, nxt, model, f0 = ref_backoff_lanes(cc, "closed form", CF_N, n_ep, 2, lanes, rows=16, slot_cap=cap,
                                                  n_bins=8)
    assert model.lost > 0
    eng, extra = _open(cc, lanes, CF_N, 1, None, 16)
    try:
        trk = LoopTrack(CF_N, 2 * lanes, log_cap=n_ep, epoch_cap=n_ep, n_bins=8)
        bo = LoopBackoff(trk, 2, slot_cap=cap)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(CF_N, dtype=torch.uint8, device="cuda") for _ in range(n_ep)]
        cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(dvcc.DvccError) as ei:
            eng.closed_loop_lanes(extra, dpool, pb, CF_N, n_ep, cursor=cursor, d_commits=commits, track=trk)
        assert ei.value.code == L.DV_ERR_ARG
        torch.cuda.synchronize()
        assert bo.counters() == model.counters() and bo.counters()[1] == model.lost
        assert np.array_equal(torch.stack(commits).cpu().numpy(), np.stack([c for c, _, _ in ref]))
        assert int(cursor.item()) == model.cur
        cnt = bo.slot_count.cpu().numpy().view(np.uint32)
        assert list(cnt) == [len(s[0]) for s in model.slots] and cnt.max() <= cap
        for (src, born, ab), (msrc, mborn, mab) in zip(bo.parked(), model.slots):
            assert np.array_equal(src, msrc) and np.array_equal(born, mborn) and np.array_equal(ab, mab)
        _guards_stand(held)
    finally:
        eng.close()


def _raw_desc(bo, n_entries, null_at=None):
    """bo's dv_loop_backoff with an aborts array of n_entries pointers (the struct keeps the array alive)"""
    ptrs = [int(bo.aborts[i % len(bo.aborts)].data_ptr()) for i in range(n_entries)]
    if null_at is not None:
        ptrs[null_at] = None
    arr = (ctypes.c_void_p * n_entries)(*ptrs)
    return L.LoopBackoffDesc(bo.n_slots, bo.slot_cap, bo.park_ids.data_ptr(), bo.park_aborts.data_ptr(),
                             bo.slot_count.data_ptr(), arr, bo.ctr.data_ptr())


def _untouched(cursor, was, trks, bos):
    torch.cuda.synchronize()
    assert int(cursor.item()) == was
    for t in trks:
        assert int(t.tot.sum().item()) == 0 and int(t.log_pos.item()) == 0
    for b in bos:
        assert sum(b.counters()) == 0 and int(b.slot_count.sum().item()) == 0


def test_refusals():
    cc = dvcc.NO_WAIT
    pool = ref_backoff_lanes(cc, POOL_KEY, N, 12, 2, 2)[0]
    f = L.lib().dv_closed_loop_backoff_lanes
    eng, (lane1, lane2) = _open(cc, 3, N, 10, 400, ROWS)
    try:
        dpool, pb = _dev_pool(pool)
        trk4 = LoopTrack(N, 4, epoch_cap=8)
        bo4 = LoopBackoff(trk4, 2)
        # ---- at attach time
        assert _code(lambda: bo4.attach(eng)) == L.DV_ERR_STATE  # no tracker attached
        assert bo4.engine is None
        trk4.attach(eng)
        d4 = _raw_desc(bo4, 2 * (MAX_LANES + 1))
        assert f(eng._ctx, ctypes.byref(d4), 0) == L.DV_ERR_ARG
        assert f(eng._ctx, ctypes.byref(d4), MAX_LANES + 1) == L.DV_ERR_ARG
        assert f(eng._ctx, None, 0) == L.DV_ERR_ARG
        assert f(eng._ctx, ctypes.byref(d4), 3) == L.DV_ERR_STATE  # a tracker of four buffers, three lanes
        assert f(eng._ctx, ctypes.byref(d4), 1) == L.DV_ERR_STATE  # (the first entry: two buffers)
        assert f(eng._ctx, ctypes.byref(_raw_desc(bo4, 4, null_at=3)), 2) == L.DV_ERR_ARG
        for name, d in malformed_descs():
            assert f(eng._ctx, ctypes.byref(d), 2) == L.DV_ERR_ARG, name
        assert _code(lambda: LoopBackoff(trk4, 3).attach(eng)) == L.DV_ERR_ARG
        with pytest.raises(ValueError):
            bo4.swap()
        cursor = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        # (nothing above attached anything: the plain tracked lanes loop's refusals aside, this would run)
        # ---- at the loop calls
        # an attachment made through the first entry (two buffers), under a tracker of four
        trk2 = LoopTrack(N, 2, epoch_cap=8)
        bo2 = LoopBackoff(trk2, 2)
        trk2.attach(eng)
        bo2.attach(eng)
        trk4.attach(eng)  # (the tracker the lanes loop needs; the back-off stays attached)
        assert _code(lambda: eng.closed_loop_lanes([lane1], dpool, pb, N, 4, cursor=cursor, track=trk4)) \
            == L.DV_ERR_STATE
        _untouched(cursor, 77, [trk2, trk4], [bo2, bo4])
        # attached for two lanes: a call over three, the single loop
        bo4.attach(eng)
        trk6 = LoopTrack(N, 6, epoch_cap=8).attach(eng)  # (the back-off stays attached)
        assert _code(lambda: eng.closed_loop_lanes([lane1, lane2], dpool, pb, N, 6, cursor=cursor, track=trk6)) \
            == L.DV_ERR_STATE
        trk2.attach(eng)
        assert _code(lambda: eng.closed_loop(dpool, pb, N, 2, cursor=cursor, track=trk2)) == L.DV_ERR_STATE
        _untouched(cursor, 77, [trk2, trk4, trk6], [bo2, bo4])
        # a back-off on a lane that is not the first
        trk4.attach(eng)
        bo4.detach()
        t1 = LoopTrack(N, 2, epoch_cap=8).attach(lane1)
        b1 = LoopBackoff(t1, 2).attach(lane1)
        assert _code(lambda: eng.closed_loop_lanes([lane1], dpool, pb, N, 4, cursor=cursor, track=trk4)) \
            == L.DV_ERR_STATE
        t1l = LoopTrack(N, 4, epoch_cap=8).attach(lane1)
        b1l = LoopBackoff(t1l, 2).attach(lane1)
        assert _code(lambda: eng.closed_loop_lanes([lane1], dpool, pb, N, 4, cursor=cursor, track=trk4)) \
            == L.DV_ERR_STATE
        _untouched(cursor, 77, [trk2, trk4, trk6, t1, t1l], [bo2, bo4, b1, b1l])
        t1l.detach()
        assert b1l.engine is None
        # detaching the tracker detaches the back-off
        bo4.attach(eng)
        trk4.detach()
        assert bo4.engine is None
    finally:
        eng.close()
    # CALVIN shares the code of a context without a tracker
    eng = dvcc.CCEngine(dvcc.CALVIN, N, N * 10)
    try:
        assert _code(lambda: LoopBackoff(LoopTrack(N, 4), 2).attach(eng)) == L.DV_ERR_STATE
    finally:
        eng.close()


def test_tpcc_loop_refuses_a_lanes_backoff():
    from dvcc import tpcc as T
    from test_tpcc_closed_loop import MAX_TXN_ACC, _params
    n, pool_n = 256, 300
    po, pp = _params(num_wh=1)
    pool = T.gen(pp, pool_n, 910)
    eng = T.TpccEngine(dvcc.WAIT_DIE, pp, n, seed=5)
    try:
        dpool, pargs = T.device_epoch(pool)
        dpool.max_txn_acc = MAX_TXN_ACC
        pb = torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()
        cursor = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        trk4 = LoopTrack(n, 4, epoch_cap=4).attach(eng)
        bo = LoopBackoff(trk4, 2).attach(eng)
        trk = LoopTrack(n, 2, epoch_cap=4).attach(eng)  # (the back-off stays attached)
        assert _code(lambda: eng.closed_loop(dpool, pargs, pb, n, 2, cursor=cursor, track=trk)) == L.DV_ERR_STATE
        _untouched(cursor, 5, [trk, trk4], [bo])
    finally:
        eng.close()


def test_a_detached_context_runs_the_plain_lanes_loop():
    cc, lanes, E = dvcc.OCC, 2, 4
    pool = ref_backoff_lanes(cc, POOL_KEY, N, 12, 2, lanes)[0]
    tab = O.YcsbTable(ROWS)
    f0 = tab.f0.copy()
    ref, nxt, cur_ref = host_closed_loop_lanes(cc, tab, f0, pool, 0, N, E, lanes)
    eng, extra = _open(cc, lanes, N, 10, 400, ROWS)
    try:
        trk = LoopTrack(N, 2 * lanes, epoch_cap=8).attach(eng)
        bo = LoopBackoff(trk, 4).attach(eng)
        bo.detach()
        bo.attach(eng)
        trk.detach()  # (and the back-off with it)
        assert bo.engine is None
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop_lanes(extra, dpool, pb, N, E, d_commits=commits)
        _check_outcomes([(c.cpu().numpy(), s) for c, s in zip(commits, sts)], ref)
        assert int(cursor.item()) == cur_ref
        for ln in range(lanes):
            _check_next(bufs[ln], 0, nxt[E + ln], N, pool)
        assert np.array_equal(eng.read_table(0, ROWS), f0)
        assert sum(bo.counters()) == 0 and int(bo.slot_count.sum().item()) == 0 and int(trk.tot.sum().item()) == 0
    finally:
        eng.close()
