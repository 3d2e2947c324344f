"""Back-off in the device closed loop on the GPU (dv_closed_loop_backoff):
the loop run under a dvcc.LoopTrack and a dvcc.LoopBackoff against
tests/test_loop_backoff.py's numpy model, driven by the oracle's commit bytes
-- never by the engine's.  Checked: every epoch's commit bytes and stats, the
epoch left in the buffers, the cursor, the table, the identity and abort
arrays of both buffers, every slot's contents and count, the tracker's log,
epoch ends, histogram and totals, and the four counters.

Shapes: 2,000 txns are seven full carry blocks of 256 and a ragged one (8,192
rows); the closed form (300 txns, one write of key 1 each, one commit per
epoch) parks 299 txns per epoch.  A spilling test asserts model.spilled > 0
first.
"""
import ctypes

import numpy as np
import pytest

from test_carry import _check_loop, _pool
from test_loop_backoff import CF_N, CF_POOL, ROWS, malformed_descs, ref_backoff

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import CCEngine, DeviceEpoch, LoopBackoff, LoopTrack  # noqa: E402
from dvcc import _lib as L  # noqa: E402

GUARD, PAD = 0xA5, 64
N, E, POOL_KEY = 2000, 24, (20000, 3)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


def _seat(t):
    """t re-seated at the head of a buffer with PAD guard elements behind it"""
    n, es = t.numel(), t.element_size()
    big = torch.full(((n + PAD) * es,), GUARD, dtype=torch.uint8, device=t.device).view(t.dtype)
    big[:n] = 0
    return big, big[:n]


def _guarded(trk, bo):
    """every array of the tracker and the back-off guarded (before attach)"""
    held = []

    def seat_attr(obj, name):
        big, view = _seat(getattr(obj, name))
        setattr(obj, name, view)
        held.append((f"{type(obj).__name__}.{name}", big, view.numel()))

    def seat_list(obj, name):
        lst = getattr(obj, name)
        for i in range(len(lst)):
            big, lst[i] = _seat(lst[i])
            held.append((f"{type(obj).__name__}.{name}[{i}]", big, lst[i].numel()))

    for name in ("log", "log_pos", "epoch_end", "hist", "tot"):
        seat_attr(trk, name)
    seat_list(trk, "ids")
    for name in ("park_ids", "park_aborts", "slot_count", "ctr"):
        seat_attr(bo, name)
    seat_list(bo, "aborts")
    return held


def _guards_stand(held):
    torch.cuda.synchronize()
    for name, big, n in held:
        assert (big[n:].view(torch.uint8) == GUARD).all(), f"{name}: written past its {n} elements"


def _dev_pool(pool):
    return DeviceEpoch(pool), torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()


def _check_outcomes(got, ref):
    for k, ((c, st), (c_ref, st_ref, host)) in enumerate(zip(got, ref)):
        assert np.array_equal(c, c_ref), k
        assert (st.n_txn, st.n_acc, st.committed) == (host.n_txn, host.n_acc, st_ref.committed), k
        assert (st.read_digest, st.write_cnt) == (st_ref.read_digest, st_ref.write_cnt), k


def _check_next(bufs, b, nxt, n_txn, pool):
    e = bufs.epoch(b, n_txn, pool.max_txn_acc())
    assert e.n_acc == nxt.n_acc
    assert np.array_equal(e.keys.cpu().numpy().view(np.uint64), nxt.keys)
    assert np.array_equal(e.types.cpu().numpy(), nxt.types)
    assert np.array_equal(e.acc_txn.cpu().numpy().view(np.uint32), nxt.acc_txn())


def _check_track(trk, model):
    torch.cuda.synchronize()
    n = len(model.epoch_end)
    assert trk.done == n
    assert list(trk.ends()) == model.epoch_end
    assert (int(trk.log_pos.item()) & 0xFFFFFFFF) == model.pos
    for i in range(n):
        src, born = trk.commits(i)
        assert np.array_equal(src.cpu().numpy(), model.log[i][0]), f"epoch {i} since attach: src"
        assert np.array_equal(born.cpu().numpy(), model.log[i][1]), f"epoch {i} since attach: born"
    assert np.array_equal(trk.histogram(), model.hist)
    assert trk.totals() == model.totals


def _check_ring(trk, bo, model, nb, n_txn):
    """the ring, the counters and both buffers' identity and abort arrays; nb:
    the buffer holding the epoch left (model.k)"""
    torch.cuda.synchronize()
    cnt = bo.slot_count.cpu().numpy().view(np.uint32)
    assert list(cnt) == [len(s[0]) for s in model.slots]
    for s, ((src, born, ab), (msrc, mborn, mab)) in enumerate(zip(bo.parked(), model.slots)):
        assert np.array_equal(src, msrc) and np.array_equal(born, mborn), f"slot {s}"
        assert np.array_equal(ab, mab.astype(np.uint8)), f"slot {s}: aborts"
    assert bo.counters() == model.counters()
    for b, k in ((nb, model.k), (nb ^ 1, model.k - 1)):
        assert np.array_equal(trk.ids[b][:n_txn].cpu().numpy(), model.words(k)), f"ids of epoch {k}"
        assert np.array_equal(bo.aborts[b][:n_txn].cpu().numpy(), model.aborts_of(k)), f"aborts of epoch {k}"


def _engine(cc, n_txn, acc, prefix, rows=ROWS):
    eng = CCEngine(cc, n_txn, n_txn * acc)
    eng.set_prefix(prefix)
    eng.load_ycsb_partition(rows)
    return eng


def _run(cc, D, prefix, pool_key, n_txn, n_epochs, rows=ROWS, acc=10, n_bins=64, slot_cap=None):
    """one call of n_epochs (even) epochs; returns what the D = 1 test compares"""
    kw = dict(n_bins=n_bins) if n_bins != 64 else {}
    pool, ref, nxt, model, f0 = ref_backoff(cc, pool_key, n_txn, n_epochs, 0, D, rows=rows, **kw)
    eng = _engine(cc, n_txn, acc, prefix, rows)
    try:
        trk = LoopTrack(n_txn, 2, log_cap=n_txn * n_epochs, epoch_cap=n_epochs, n_bins=n_bins)
        bo = LoopBackoff(trk, D, slot_cap=slot_cap)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(n_txn, dtype=torch.uint8, device="cuda") for _ in range(n_epochs)]
        sts, bufs, cursor = eng.closed_loop(dpool, pb, n_txn, n_epochs, d_commits=commits, track=trk)
        got = [(c.cpu().numpy(), s) for c, s in zip(commits, sts)]
        _check_outcomes(got, ref)
        assert int(cursor.item()) == model.cur
        _check_next(bufs, 0, nxt, n_txn, pool)
        assert np.array_equal(eng.read_table(0, rows), f0)
        _check_track(trk, model)
        _check_ring(trk, bo, model, 0, n_txn)
        _guards_stand(held)
        e = bufs.epoch(0, n_txn, acc)
        return dict(commits=np.stack([c for c, _ in got]), cursor=int(cursor.item()), log=trk.log.cpu().numpy(),
                    ends=trk.ends(), hist=trk.histogram(), totals=trk.totals(),
                    ids=[t[:n_txn].cpu().numpy() for t in trk.ids], keys=e.keys.cpu().numpy(),
                    acc_txn=e.acc_txn.cpu().numpy(), types=e.types.cpu().numpy())
    finally:
        eng.close()


@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC])
@pytest.mark.parametrize("D", [1, 2, 4, 8])
@pytest.mark.parametrize("prefix", [400, None])
def test_random_shape(cc, D, prefix):
    """2,000 txns on 8,192 rows, 24 epochs: the pipelined tb-form loop (prefix
    400) and epochs one at a time in the keys form (prefix off)"""
    model = ref_backoff(cc, POOL_KEY, N, E, 0, D)[3]
    if D in (2, 4, 8):
        assert model.spilled > 0
    assert model.totals[3] >= 1 and model.lost == 0
    _run(cc, D, prefix, POOL_KEY, N, E)


def test_random_shape_longest_delay_16():
    """all five delay classes: a txn's fifth abort parks it 16 epochs ahead"""
    model = ref_backoff(dvcc.NO_WAIT, POOL_KEY, N, E, 0, 16)[3]
    assert model.spilled > 0 and model.totals[3] >= 4 and any((s[2] >= 5).any() for s in model.slots)
    _run(dvcc.NO_WAIT, 16, 400, POOL_KEY, N, E)


@pytest.mark.parametrize("prefix", [400, None])
def test_d1_equals_the_plain_tracked_loop(prefix):
    cc = dvcc.NO_WAIT
    got = _run(cc, 1, prefix, POOL_KEY, N, E)
    pool = ref_backoff(cc, POOL_KEY, N, E, 0, 1)[0]
    eng = _engine(cc, N, 10, prefix)
    try:
        trk = LoopTrack(N, 2, log_cap=N * E, epoch_cap=E, n_bins=64).attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop(dpool, pb, N, E, d_commits=commits, track=trk)
        torch.cuda.synchronize()
        assert np.array_equal(torch.stack(commits).cpu().numpy(), got["commits"])
        assert int(cursor.item()) == got["cursor"]
        assert np.array_equal(trk.log.cpu().numpy(), got["log"]) and list(trk.ends()) == list(got["ends"])
        assert np.array_equal(trk.histogram(), got["hist"]) and trk.totals() == got["totals"]
        for b in range(2):
            assert np.array_equal(trk.ids[b][:N].cpu().numpy(), got["ids"][b])
        e = bufs.epoch(0, N, 10)
        assert np.array_equal(e.keys.cpu().numpy(), got["keys"]) and np.array_equal(e.types.cpu().numpy(), got["types"])
        assert np.array_equal(e.acc_txn.cpu().numpy(), got["acc_txn"])
    finally:
        eng.close()


@pytest.mark.parametrize("D", [2, 8])
def test_closed_form(D):
    model = ref_backoff(dvcc.NO_WAIT, "closed form", CF_N, 40, 0, D, rows=16)[3]
    assert model.spilled > 0 and model.cur == sum(len(d) for d in model.drawn) % CF_POOL
    _run(dvcc.NO_WAIT, D, None, "closed form", CF_N, 40, rows=16, acc=1, n_bins=8)


def test_forced_yields_swaps_and_reattach():
    """asynchronous launches forced to yield (every epoch halts: the refill
    queued behind it is a no-op and is queued again after the synchronous
    decision), three calls of 3 epochs with the three swaps between them, then
    a drained log attached again at epoch 9"""
    cc, n, D, calls, per = dvcc.NO_WAIT, 3000, 4, 3, 3
    total = calls * per + per
    pool_key = (4000, 12, 12)
    pool, ref, nxt, final, f0 = ref_backoff(cc, pool_key, n, total, 0, D, n_bins=16)
    eng = _engine(cc, n, 12, 500)
    try:
        eng.set_async_limits(1, 0)
        trk = LoopTrack(n, 2, log_cap=n * total, epoch_cap=calls * per, n_bins=16)
        bo = LoopBackoff(trk, D)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(per)]
        cursor, bufs, got, yields = None, None, [], 0
        for call in range(calls + 1):
            if call == calls:
                trk.drain()
                trk.attach(eng, first_epoch=calls * per)
            sts, bufs, cursor = eng.closed_loop(dpool, pb, n, per, cursor=cursor, bufs=bufs, d_commits=commits,
                                                resume=call > 0, track=trk)
            got += [(c.cpu().numpy().copy(), s) for c, s in zip(commits, sts)]
            yields += sum(s.async_yields for s in sts)
            bufs.swap()
            trk.swap()
            bo.swap()
            # the model after the same epochs (its own run: the cached one is read-only)
            m = ref_backoff(cc, pool_key, n, (call + 1) * per, 0, D, n_bins=16)[3]
            assert np.array_equal(trk.ids[0][:n].cpu().numpy(), m.words(m.k)), call
            assert np.array_equal(bo.aborts[0][:n].cpu().numpy(), m.aborts_of(m.k)), call
            assert bo.counters() == m.counters(), call
        assert yields > 0, "no asynchronous launch yielded"
        assert final.spilled > 0
        _check_outcomes(got, ref)
        assert int(cursor.item()) == final.cur
        _check_next(bufs, 0, nxt, n, pool)
        assert np.array_equal(eng.read_table(0, ROWS), f0)
        _check_ring(trk, bo, final, 0, n)
        # the tracker since the second attach: the last three epochs' log
        assert list(trk.ends()) == [e - final.epoch_end[calls * per - 1] for e in final.epoch_end[calls * per:]]
        for i in range(per):
            src, born = trk.commits(i)
            assert np.array_equal(src.cpu().numpy(), final.log[calls * per + i][0]), i
            assert np.array_equal(born.cpu().numpy(), final.log[calls * per + i][1]), i
        assert np.array_equal(trk.histogram(), final.hist) and trk.totals() == final.totals
        _guards_stand(held)
    finally:
        eng.close()


def test_capacity_exceeded():
    """closed form, D = 2, 300 entries a slot where the model reaches 597"""
    cc, n_ep, cap = dvcc.NO_WAIT, 40, 300
    assert ref_backoff(cc, "closed form", CF_N, n_ep, 0, 2, rows=16)[3].fullest > cap
    pool, ref, nxt, model, f0 = ref_backoff(cc, "closed form", CF_N, n_ep, 0, 2, rows=16, slot_cap=cap, n_bins=8)
    assert model.lost > 0
    eng = _engine(cc, CF_N, 1, None, 16)
    try:
        trk = LoopTrack(CF_N, 2, log_cap=n_ep, epoch_cap=n_ep, n_bins=8)
        bo = LoopBackoff(trk, 2, slot_cap=cap)
        held = _guarded(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(CF_N, dtype=torch.uint8, device="cuda") for _ in range(n_ep)]
        cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(dvcc.DvccError) as ei:
            eng.closed_loop(dpool, pb, CF_N, n_ep, cursor=cursor, d_commits=commits, track=trk)
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


def _code(call):
    with pytest.raises(dvcc.DvccError) as ei:
        call()
    return ei.value.code


def test_refusals():
    cc = dvcc.NO_WAIT
    pool = ref_backoff(cc, POOL_KEY, N, E, 0, 2)[0]
    eng = _engine(cc, N, 10, 400)
    try:
        dpool, pb = _dev_pool(pool)
        trk = LoopTrack(N, 2, epoch_cap=8)
        assert _code(lambda: LoopBackoff(trk, 2).attach(eng)) == L.DV_ERR_STATE  # no tracker attached
        trk.attach(eng)
        assert _code(lambda: LoopBackoff(trk, 3).attach(eng)) == L.DV_ERR_ARG
        for name, d in malformed_descs():
            assert L.lib().dv_closed_loop_backoff(eng._ctx, ctypes.byref(d)) == L.DV_ERR_ARG, name
        # the lanes loop with a back-off attached to the first lane
        trk.detach()
        lane = eng.open_lane()
        trk4 = LoopTrack(N, 4, epoch_cap=8).attach(eng)
        trk2 = LoopTrack(N, 2, epoch_cap=8)
        bo = LoopBackoff(trk2, 2)
        trk2.attach(eng)
        bo.attach(eng)
        trk4.attach(eng)  # (the tracker the lanes loop needs; the back-off stays attached)
        cursor = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        assert _code(lambda: eng.closed_loop_lanes([lane], dpool, pb, N, 4, cursor=cursor, track=trk4)) \
            == L.DV_ERR_STATE
        torch.cuda.synchronize()
        assert int(cursor.item()) == 77 and int(trk4.tot.sum().item()) == 0 and int(trk4.log_pos.item()) == 0
        assert sum(bo.counters()) == 0 and int(bo.slot_count.sum().item()) == 0
        # detaching the tracker detaches the back-off: the plain loop, as tests/test_carry.py checks it
        trk4.detach()
        assert bo.engine is None
    finally:
        eng.close()
    # CALVIN and a context without a tracker share the code
    eng = CCEngine(dvcc.CALVIN, N, N * 10)
    try:
        assert _code(lambda: LoopBackoff(LoopTrack(N, 2), 2).attach(eng)) == L.DV_ERR_STATE
    finally:
        eng.close()


def test_tpcc_loop_refuses_a_backoff():
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
        trk = LoopTrack(n, 2, epoch_cap=4).attach(eng)
        bo = LoopBackoff(trk, 2).attach(eng)
        assert _code(lambda: eng.closed_loop(dpool, pargs, pb, n, 2, cursor=cursor, track=trk)) == L.DV_ERR_STATE
        torch.cuda.synchronize()
        assert int(cursor.item()) == 5 and int(trk.tot.sum().item()) == 0 and int(trk.log_pos.item()) == 0
        assert sum(bo.counters()) == 0 and int(bo.slot_count.sum().item()) == 0
    finally:
        eng.close()


def test_a_detached_context_runs_the_plain_loop():
    cc = dvcc.OCC
    pool = _pool(ROWS, 5000, 11)
    eng = _engine(cc, N, 10, 400)
    try:
        trk = LoopTrack(N, 2, epoch_cap=8).attach(eng)
        bo = LoopBackoff(trk, 4).attach(eng)
        bo.detach()
        bo.attach(eng)
        trk.detach()  # (and the back-off with it)
        assert bo.engine is None
        _check_loop(eng, cc, ROWS, pool, N, 6, cur0=1234)
        assert sum(bo.counters()) == 0 and int(bo.slot_count.sum().item()) == 0 and int(trk.tot.sum().item()) == 0
    finally:
        eng.close()
