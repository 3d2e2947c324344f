"""The loop tracker on the GPU (dv_closed_loop_track): every closed loop run
under a dvcc.LoopTrack, its commit log, epoch ends, histogram, totals and
identity buffers against tests/test_loop_track.py's numpy model, driven by the
oracle's commit bytes (tests/test_carry.py's host loops, TpccDB.epoch) -- never
by the engine's.  The loops' own results (commit bytes, stats, cursor, next
epoch, table) are checked as tests/test_carry.py and
tests/test_tpcc_closed_loop.py check them.

Shapes: 2,000 txns are seven full carry blocks of 256 and a ragged one; the
closed form (300 txns, one commit per epoch) has a block with nothing
committed and a block with nothing carried but its first txn.
"""
import ctypes
import struct

import numpy as np
import pytest

import _oracle as O
import wire_fmt as W
import test_wire_device_cases as C
from test_carry import _pool, host_closed_loop, host_closed_loop_lanes
from test_loop_track import (CF_E, CF_N, CF_POOL, TrackModel, closed_form, closed_form_commits, closed_form_pool,
                             malformed_descs)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import CCEngine, DeviceEpoch, LoopTrack  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc.wire import DeviceWireIngress, WireIngress  # noqa: E402

ROWS = 1 << 13
GUARD, PAD = 0xA5, 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


_ref_cache = {}


def _ref_single(cc, pool_key, n_txn, n_epochs, cur0):
    """the oracle's single loop (computed once per shape, read-only afterwards)"""
    key = ("single", cc, pool_key, n_txn, n_epochs, cur0)
    if key not in _ref_cache:
        pool = _pool(ROWS, *pool_key)
        tab = O.YcsbTable(ROWS)
        f0 = tab.f0.copy()
        ref, nxt, cur = host_closed_loop(cc, tab, f0, pool, cur0, n_txn, n_epochs)
        _ref_cache[key] = (pool, ref, nxt, cur, f0)
    return _ref_cache[key]


def _ref_lanes(cc, pool_key, n_txn, n_epochs, lanes):
    key = ("lanes", cc, pool_key, n_txn, n_epochs, lanes)
    if key not in _ref_cache:
        pool = _pool(ROWS, *pool_key)
        tab = O.YcsbTable(ROWS)
        f0 = tab.f0.copy()
        ref, nxt, cur = host_closed_loop_lanes(cc, tab, f0, pool, 0, n_txn, n_epochs, lanes)
        _ref_cache[key] = (pool, ref, nxt, cur, f0)
    return _ref_cache[key]


def _model_matches_epochs(model, ref, pool):
    """the model's identities name the oracle's epochs: epoch k's txn t holds
    the accesses of pool txn src[t]"""
    tb = pool.txn_begin.astype(np.int64)
    for k, (_, _, host) in enumerate(ref):
        src = model.seen[model.k - len(ref) + k][0]
        assert np.array_equal(host.keys[host.txn_begin[:-1].astype(np.int64)], pool.keys[tb[src]]), k


def _guarded(trk):
    """every tracker array re-seated at the head of a buffer with PAD guard
    elements behind it (before attach)"""
    held = {}

    def seat(t):
        n, es = t.numel(), t.element_size()
        big = torch.full(((n + PAD) * es,), GUARD, dtype=torch.uint8, device=t.device).view(t.dtype)
        big[:n] = 0
        return big, big[:n]

    for name in ("log", "log_pos", "epoch_end", "hist", "tot"):
        held[name], view = seat(getattr(trk, name))
        setattr(trk, name, view)
    for i in range(trk.n_bufs):
        held[f"ids{i}"], trk.ids[i] = seat(trk.ids[i])
    return held


def _guards_stand(trk, held):
    torch.cuda.synchronize()
    for name, big in held.items():
        n = trk.ids[0].numel() if name.startswith("ids") else getattr(trk, name).numel()
        assert (big[n:].view(torch.uint8) == GUARD).all(), f"{name}: written past its {n} elements"


def _check_track(trk, model, first=0):
    """the tracker's tensors against the model: epochs first.. since attach"""
    torch.cuda.synchronize()
    n = len(model.epoch_end)
    assert trk.done == n
    assert list(trk.ends()) == model.epoch_end
    assert (int(trk.log_pos.item()) & 0xFFFFFFFF) == model.pos
    for i in range(first, n):
        src, born = trk.commits(i)
        assert np.array_equal(src.cpu().numpy(), model.log[i][0]), f"epoch {i} since attach: src"
        assert np.array_equal(born.cpu().numpy(), model.log[i][1]), f"epoch {i} since attach: born"
    assert np.array_equal(trk.histogram(), model.hist)
    assert trk.totals() == model.totals


def _check_outcomes(got, ref):
    for k, ((c, st), (c_ref, st_ref, host)) in enumerate(zip(got, ref)):
        assert np.array_equal(c, c_ref), k
        assert (st.n_txn, st.n_acc, st.committed) == (host.n_txn, host.n_acc, st_ref.committed), k
        assert (st.read_digest, st.write_cnt) == (st_ref.read_digest, st_ref.write_cnt), k


def _check_next(bufs, nxt, n_txn, pool):
    e = bufs.epoch(0, n_txn, pool.max_txn_acc())
    assert e.n_acc == nxt.n_acc
    assert np.array_equal(e.keys.cpu().numpy().view(np.uint64), nxt.keys)
    assert np.array_equal(e.types.cpu().numpy(), nxt.types)
    assert np.array_equal(e.acc_txn.cpu().numpy().view(np.uint32), nxt.acc_txn())


def _dev_pool(pool):
    return DeviceEpoch(pool), torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()


def _ids(trk, b, n):
    return trk.ids[b][:n].cpu().numpy()


@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC])
@pytest.mark.parametrize("prefix", [None, 400])
def test_single_loop_tracked(cc, prefix):
    """one call of 6 epochs from cursor 1234, epochs one at a time (prefix
    off) and the pipelined tb-form loop (prefix 400)"""
    N, E, cur0 = 2000, 6, 1234
    pool, ref, nxt, cur_ref, f0 = _ref_single(cc, (5000, 11), N, E, cur0)
    model = TrackModel(pool.n_txn, cur0, N)
    for c, _, _ in ref:
        model.epoch(c)
    assert model.cur == cur_ref
    _model_matches_epochs(model, ref, pool)
    eng = CCEngine(cc, N, N * 10)
    try:
        eng.set_prefix(prefix)
        eng.load_ycsb_partition(ROWS)
        trk = LoopTrack(N, 2, log_cap=N * E, epoch_cap=E, n_bins=64)
        held = _guarded(trk)
        trk.attach(eng)
        dpool, pb = _dev_pool(pool)
        cursor = torch.full((1,), cur0, dtype=torch.int32, device="cuda")
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop(dpool, pb, N, E, cursor=cursor, d_commits=commits, track=trk)
        _check_outcomes([(c.cpu().numpy(), s) for c, s in zip(commits, sts)], ref)
        assert int(cursor.item()) == cur_ref
        _check_next(bufs, nxt, N, pool)
        assert np.array_equal(eng.read_table(0, ROWS), f0)
        _check_track(trk, model)
        assert trk.overflowed() == 0
        assert np.array_equal(_ids(trk, E & 1, N), model.words(E))
        assert np.array_equal(_ids(trk, (E - 1) & 1, N), model.words(E - 1))
        _guards_stand(trk, held)
    finally:
        eng.close()


def test_closed_form_on_the_device():
    """every pool txn one write of key 1 (tests/test_loop_track.py): epoch k
    commits pool txn k, born max(0, k - N + 1), after min(k, N - 1) retries;
    8 bins, so the last one saturates"""
    commits_ref = closed_form_commits()
    want, retries, totals, hist = closed_form(8)
    pool = closed_form_pool()
    eng = CCEngine(dvcc.NO_WAIT, CF_N, CF_N)
    try:
        eng.set_prefix(None)
        eng.load_ycsb_partition(16)
        trk = LoopTrack(CF_N, 2, log_cap=CF_E, epoch_cap=CF_E, n_bins=8).attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(CF_N, dtype=torch.uint8, device="cuda") for _ in range(CF_E)]
        sts, bufs, cursor = eng.closed_loop(dpool, pb, CF_N, CF_E, d_commits=commits, track=trk)
        torch.cuda.synchronize()
        got = torch.stack(commits).cpu().numpy()
        assert np.array_equal(got, np.stack(commits_ref))
        assert int(cursor.item()) == (CF_N + CF_E) % CF_POOL
        assert list(trk.ends()) == list(range(1, CF_E + 1)) and int(trk.log_pos.item()) == CF_E
        log = trk.log.cpu().numpy()
        assert np.array_equal(log & 0xFFFFFFFF, np.array([s for s, _ in want]))
        assert np.array_equal(log >> 32, np.array([b for _, b in want]))
        src, born = trk.commits(CF_E - 1)
        assert (src.tolist(), born.tolist()) == ([CF_E - 1], [CF_E - CF_N])
        assert trk.totals() == totals
        assert np.array_equal(trk.histogram(), hist) and hist[7] == CF_E - 7
        # the epoch left: the queue's CF_N - 1 waiting txns, oldest first, and one fresh txn
        nxt = _ids(trk, CF_E & 1, CF_N)
        assert np.array_equal(nxt & 0xFFFFFFFF, CF_E + np.arange(CF_N))
        assert np.array_equal(nxt >> 32, np.arange(CF_E - CF_N + 1, CF_E + 1))
    finally:
        eng.close()


def test_forced_yields_resume_and_reattach():
    """asynchronous launches forced to yield (every epoch halts: its refill
    and the tracker pass behind it are no-ops, both queued again after the
    synchronous decision), three calls of 3 epochs with the buffers swapped
    between them, then a drained log attached again at epoch 9"""
    cc, N, calls, per = dvcc.NO_WAIT, 3000, 3, 3
    total = calls * per + per
    pool, ref, nxt, cur_ref, f0 = _ref_single(cc, (4000, 12, 12), N, total, 0)
    model = TrackModel(pool.n_txn, 0, N, n_bins=16)
    eng = CCEngine(cc, N, N * 12)
    try:
        eng.set_prefix(500)
        eng.set_async_limits(1, 0)
        eng.load_ycsb_partition(ROWS)
        trk = LoopTrack(N, 2, log_cap=N * total, epoch_cap=calls * per, n_bins=16).attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(per)]
        cursor, bufs, got, yields = None, None, [], 0
        for call in range(calls + 1):
            if call == calls:  # a drained log, the identities continued
                _check_track(trk, model)
                trk.drain()
                model.drain()
                trk.attach(eng, first_epoch=calls * per)
            sts, bufs, cursor = eng.closed_loop(dpool, pb, N, per, cursor=cursor, bufs=bufs, d_commits=commits,
                                                resume=call > 0, track=trk)
            got += [(c.cpu().numpy().copy(), s) for c, s in zip(commits, sts)]
            yields += sum(s.async_yields for s in sts)
            for c, _, _ in ref[call * per:(call + 1) * per]:
                model.epoch(c)
            bufs.swap()
            trk.swap()
            k = (call + 1) * per  # the next epoch, now in buffer 0
            assert np.array_equal(_ids(trk, 0, N), model.words(k)), call
            assert np.array_equal(_ids(trk, 1, N), model.words(k - 1)), call
        assert yields > 0, "no asynchronous launch yielded"
        _check_outcomes(got, ref)
        assert int(cursor.item()) == cur_ref
        _check_next(bufs, nxt, N, pool)
        assert np.array_equal(eng.read_table(0, ROWS), f0)
        _check_track(trk, model)  # (three epochs since the second attach)
        born = np.concatenate([b for _, b in model.log])
        assert born.min() < calls * per <= born.max()  # commits born before and after the re-attachment
    finally:
        eng.close()


def _run_lanes(cc, lanes, prefix, N, n_epochs, calls, pool_key, async_iters=None):
    total = n_epochs * calls
    pool, ref, nxt, cur_ref, f0 = _ref_lanes(cc, pool_key, N, total, lanes)
    model = TrackModel(pool.n_txn, 0, N, lanes=lanes, n_bins=16)
    for c, _, _ in ref:
        model.epoch(c)
    assert model.cur == cur_ref
    eng = CCEngine(cc, N, N * pool.max_txn_acc())
    eng.set_prefix(prefix)
    eng.load_ycsb_partition(ROWS)
    extra = [eng.open_lane() for _ in range(lanes - 1)]
    if async_iters:
        for e in [eng] + extra:
            e.set_async_limits(async_iters, 0)
    try:
        trk = LoopTrack(N, 2 * lanes, log_cap=N * total, epoch_cap=total, n_bins=16)
        held = _guarded(trk)
        trk.attach(eng)
        dpool, pb = _dev_pool(pool)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(n_epochs)]
        cursor, bufs, got = None, None, []
        for call in range(calls):
            sts, bufs, cursor = eng.closed_loop_lanes(extra, dpool, pb, N, n_epochs, cursor=cursor, bufs=bufs,
                                                      d_commits=commits, resume=call > 0, track=trk)
            got += [(c.cpu().numpy().copy(), s) for c, s in zip(commits, sts)]
        _check_outcomes(got, ref)
        assert int(cursor.item()) == cur_ref
        assert np.array_equal(eng.read_table(0, ROWS), f0)
        _check_track(trk, model)  # (the log in epoch order; the model asserts (k - born) % L == 0)
        for k, (_, born) in enumerate(model.log):
            assert ((k - born) % lanes == 0).all()
        assert total % (2 * lanes) == 0  # every lane's next epoch in its first buffer
        for ln in range(lanes):
            assert np.array_equal(_ids(trk, 2 * ln, N), model.words(total + ln)), ln
            assert np.array_equal(_ids(trk, 2 * ln + 1, N), model.words(total - lanes + ln)), ln
        _guards_stand(trk, held)
        return trk, model
    finally:
        eng.close()


@pytest.mark.parametrize("cc,lanes,prefix", [(dvcc.NO_WAIT, 2, 400), (dvcc.NO_WAIT, 3, None), (dvcc.WAIT_DIE, 4, 400)])
def test_lanes_tracked(cc, lanes, prefix):
    """epoch k on lane k % L, an abort back L epochs later: the log in epoch
    order and retries (k - born) / L"""
    trk, model = _run_lanes(cc, lanes, prefix, 2000, 4 * lanes, 1, (5000, 21))  # (a multiple of 2 L epochs)
    assert model.totals[3] >= 1  # some txn committed on a retry
    assert trk.histogram()[1:].sum() > 0


def test_lanes_tracked_forced_yields_two_calls():
    _run_lanes(dvcc.NO_WAIT, 2, 500, 3000, 4, 2, (4000, 22, 12), async_iters=1)


def test_log_overflow_is_counted_not_written():
    cc, N, E, cur0 = dvcc.NO_WAIT, 2000, 6, 1234
    pool, ref, nxt, cur_ref, f0 = _ref_single(cc, (5000, 11), N, E, cur0)
    full = TrackModel(pool.n_txn, cur0, N)
    for c, _, _ in ref:
        full.epoch(c)
    cap = full.epoch_end[2] + 3
    assert full.epoch_end[2] < cap < full.epoch_end[3] < full.pos  # the cap cuts inside epoch 3
    eng = CCEngine(cc, N, N * 10)
    try:
        eng.set_prefix(None)
        eng.load_ycsb_partition(ROWS)
        trk = LoopTrack(N, 2, log_cap=cap, epoch_cap=E, n_bins=64)
        held = _guarded(trk)
        trk.attach(eng)
        dpool, pb = _dev_pool(pool)
        cursor = torch.full((1,), cur0, dtype=torch.int32, device="cuda")
        eng.closed_loop(dpool, pb, N, E, cursor=cursor, track=trk)
        torch.cuda.synchronize()
        full.log_cap = cap
        assert np.array_equal(trk.log.cpu().numpy(), full.log_words())
        assert list(trk.ends()) == full.epoch_end and (int(trk.log_pos.item()) & 0xFFFFFFFF) == full.pos
        assert trk.overflowed() == full.pos - cap
        assert trk.commits(3)[0].numel() == 3 and trk.commits(4)[0].numel() == 0
        assert np.array_equal(trk.histogram(), full.hist) and trk.totals() == full.totals
        _guards_stand(trk, held)
    finally:
        eng.close()


def test_refusals_and_detach():
    cc, N, E, cur0 = dvcc.NO_WAIT, 2000, 6, 1234
    pool, ref, nxt, cur_ref, f0 = _ref_single(cc, (5000, 11), N, E, cur0)
    dpool, pb = _dev_pool(pool)

    def code(call):
        with pytest.raises(dvcc.DvccError) as ei:
            call()
        return ei.value.code

    eng = CCEngine(cc, N, N * 10)
    try:
        eng.set_prefix(400)
        eng.load_ycsb_partition(ROWS)
        lane = eng.open_lane()
        for name, d in malformed_descs():
            assert L.lib().dv_closed_loop_track(eng._ctx, ctypes.byref(d)) == L.DV_ERR_ARG, name
        trk = LoopTrack(N, 2, epoch_cap=4).attach(eng)
        cursor = torch.full((1,), cur0, dtype=torch.int32, device="cuda")
        # a two-lane call (four buffers) under a tracker of two: refused at the C entry
        bufs4 = [dvcc.ClosedLoopBufs(N * 10, False, "cuda", n_txn=N) for _ in range(2)]
        arr = (L.EpochDev * 4)(*[b.desc(i) for b in bufs4 for i in range(2)])
        lp = (ctypes.c_void_p * 2)(eng._ctx.value, lane._ctx.value)
        rc = L.lib().dv_epoch_run_closed_loop_lanes(lp, 2, ctypes.byref(dpool.desc()), pb.data_ptr(),
                                                    cursor.data_ptr(), N, arr, N * 10, 4, 0, None, None)
        assert rc == L.DV_ERR_ARG
        with pytest.raises(ValueError):  # (and by the Python wrapper before it)
            eng.closed_loop_lanes([lane], dpool, pb, N, 4, cursor=cursor, track=trk)
        # more epochs than the attachment may run
        assert code(lambda: eng.closed_loop(dpool, pb, N, 5, cursor=cursor, track=trk)) == L.DV_ERR_ARG
        torch.cuda.synchronize()
        assert int(cursor.item()) == cur0 and trk.done == 0  # nothing was launched
        assert int(trk.tot.sum().item()) == 0 and int(trk.log_pos.item()) == 0
        # after detach: the loop as on a fresh engine, the tracker untouched
        trk.detach()
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop(dpool, pb, N, E, cursor=cursor, d_commits=commits)
        got = [(c.cpu().numpy(), s) for c, s in zip(commits, sts)]
        _check_outcomes(got, ref)
        fresh = CCEngine(cc, N, N * 10)
        try:
            fresh.set_prefix(400)
            fresh.load_ycsb_partition(ROWS)
            c2 = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
            cur2 = torch.full((1,), cur0, dtype=torch.int32, device="cuda")
            _, bufs2, cur2 = fresh.closed_loop(dpool, pb, N, E, cursor=cur2, d_commits=c2)
            for a, b in zip(commits, c2):
                assert torch.equal(a, b)
            assert int(cursor.item()) == int(cur2.item()) == cur_ref
            e1, e2 = bufs.epoch(0, N, 10), bufs2.epoch(0, N, 10)
            assert e1.n_acc == e2.n_acc and torch.equal(e1.keys, e2.keys) and torch.equal(e1.acc_txn, e2.acc_txn)
        finally:
            fresh.close()
        _check_next(bufs, nxt, N, pool)
        assert int(trk.tot.sum().item()) == 0 and int(trk.log_pos.item()) == 0 and int(trk.ids[0].sum().item()) == 0
    finally:
        eng.close()
    # CALVIN never aborts: refused at attach time with the loop's own code
    eng = CCEngine(dvcc.CALVIN, N, N * 10)
    try:
        assert code(lambda: LoopTrack(N, 2).attach(eng)) == L.DV_ERR_STATE
    finally:
        eng.close()


def test_tpcc_loop_tracked():
    """WAIT_DIE over 4 warehouses, 1,000 txns per epoch (four carry blocks, the
    last ragged), the pool wrapping in the first take"""
    from dvcc import tpcc as T
    from test_tpcc_carry import host_carry, host_concat, host_take
    from test_tpcc_closed_loop import MAX_TXN_ACC, _params, _ref, _same_epoch, _same_outcome
    cc, N, POOL, CUR0, E = dvcc.WAIT_DIE, 1000, 1200, 900, 5
    po, pp = _params(num_wh=4)
    db = O.TpccDB(po, 5)
    pool = T.gen(pp, POOL, 910)
    model = TrackModel(POOL, CUR0, N, n_bins=8)
    host, cur, ref = host_take(pool, CUR0, N), (CUR0 + N) % POOL, []
    for _ in range(E):
        c_ref, o_ref, st_ref = _ref(db, cc, host)
        ref.append((c_ref, o_ref, st_ref, host))
        model.epoch(c_ref)
        hc = host_carry(host, c_ref, N)
        host = host_concat(hc, host_take(pool, cur, N - hc.n_txn))
        cur = (cur + N - hc.n_txn) % POOL
    assert model.cur == cur and model.totals[3] >= 1
    eng = T.TpccEngine(cc, pp, N, seed=5)
    try:
        dpool, pargs = T.device_epoch(pool)
        dpool.max_txn_acc = MAX_TXN_ACC
        pb = torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()
        cursor = torch.full((1,), CUR0, dtype=torch.int32, device="cuda")
        trk = LoopTrack(N, 2, log_cap=N * E, epoch_cap=E, n_bins=8)
        held = _guarded(trk)
        trk.attach(eng)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        oids = [torch.zeros(N, dtype=torch.int64, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop(dpool, pargs, pb, N, E, cursor=cursor, d_commits=commits, d_oids=oids,
                                            track=trk)
        for k, (c, o, st) in enumerate(zip(commits, oids, sts)):
            _same_outcome(k, c.cpu().numpy(), o.cpu().numpy().view(np.uint64), st, *ref[k])
        assert int(cursor.item()) == cur
        bufs.swap()  # (E odd: the next epoch to buffer 0)
        trk.swap()
        e, e_args = bufs.epoch(0, N, MAX_TXN_ACC)
        _same_epoch(e, e_args, host, "the epoch left in the buffers")
        for t in range(5):
            ref_t = db.table(t)
            for col in range(3):
                assert (eng.read_col(t, col) == ref_t[1 + col]).all(), f"table {t} col {col}"
        _check_track(trk, model)
        assert np.array_equal(_ids(trk, 0, N), model.words(E))
        _guards_stand(trk, held)
    finally:
        eng.close()


def _client_streams(rows, n_per, seeds):
    """three clients' batches interleaved as they arrive, back to back"""
    g = dvcc.YCSBQueryGenerator(rows, zipf_theta=0.9, txn_write_perc=1.0, tup_write_perc=0.5)
    streams = [W.batches(0, 1 + c, W.ycsb_epoch_messages(g.gen(n_per, s),
                                                         client_startts=100_000 * c + np.arange(n_per)))
               for c, s in enumerate(seeds)]
    out = []
    for i in range(max(len(s) for s in streams)):
        out += [s[i] for s in streams if i < len(s)]
    return out


def _reply_batches(node_id, txn_id, client_startts, return_node):
    """wire_fmt's encoding of the CL_RSP batches for these txns, in this
    order: one run of batches per destination, destinations ascending (the
    reference's per-destination mbufs)"""
    out = []
    for dest in sorted(set(int(r) for r in return_node)):
        msgs = [W.header(W.CL_RSP, int(t)) + struct.pack("<Q", int(c))
                for t, c, r in zip(txn_id, client_startts, return_node) if int(r) == dest]
        out += W.batches(dest, node_id, msgs)
    return out


def test_replies_at_commit_end_to_end():
    """a client stream ingested on the device is the loop's pool; every
    epoch's log slice answers its commits, whatever epoch they were born in"""
    cc, N, E, n_per = dvcc.NO_WAIT, 1000, 5, 800
    batches = _client_streams(ROWS, n_per, (70, 71, 72))
    buf, off = C.stream(batches)
    host = WireIngress(L.YCSB, 4000, 40_000, node_id=0, node_cnt=1, synth_table_size=ROWS)
    assert host.feed_buffer(buf, off) == []
    pool = host.take()
    assert pool.n_txn == 3 * n_per and len(set(pool.return_node.tolist())) == 3
    tab = O.YcsbTable(ROWS)
    f0 = tab.f0.copy()
    ref, nxt, cur_ref = host_closed_loop(cc, tab, f0, pool, 0, N, E)
    model = TrackModel(pool.n_txn, 0, N)
    for c, _, _ in ref:
        model.epoch(c)
    assert N + model.epoch_end[E - 2] <= pool.n_txn, "the pool wraps: a txn would be answered twice by right"
    assert model.totals[3] >= 1
    eng = CCEngine(cc, 4000, 40_000)
    try:
        eng.set_prefix(None)
        eng.load_ycsb_partition(ROWS)
        ing = DeviceWireIngress(eng, 4000, 40_000, node_id=0, node_cnt=1, synth_table_size=ROWS)
        dep, taken, status = ing.feed_buffer(buf, off)
        assert (taken, status, dep.n_txn) == (len(batches), L.DV_OK, pool.n_txn)
        trk = LoopTrack(N, 2, log_cap=N * E, epoch_cap=E).attach(eng)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop(dep, ing.txn_begin, N, E, d_commits=commits, track=trk)
        _check_outcomes([(c.cpu().numpy(), s) for c, s in zip(commits, sts)], ref)
        _check_track(trk, model)
        answered = []
        for i in range(E):
            src = model.log[i][0]
            want = _reply_batches(0, pool.txn_id[src], pool.client_startts[src], pool.return_node[src])
            got = ing.respond_logged(trk.commits(i)[0])
            assert got == want, i
            answered += [m["txn_id"] for b in got for m in W.parse_batch(b)[2]]
        assert len(answered) == model.pos and len(set(answered)) == len(answered)
        assert ing.respond_logged(trk.commits(0)[0][:0]) == []
    finally:
        eng.close()
