"""Retries of aborted TPC-C txns on the device: dv_tpcc_epoch_carry,
dv_tpcc_epoch_run_closed_loop and TPC-C epochs whose access count lives on the
device (dv_epoch_dev::n_acc_dev).

The reference is the oracle's TpccDB.epoch run in a host closed loop built
from tests/test_tpcc_carry.py's numpy rule.  Integer work, so everything is
compared bit for bit: commit bytes, the o_id of every committed NewOrder,
the per-epoch stats, the carried epoch's five arrays, the cursor and every
column of every table.
"""
import numpy as np
import pytest

import _oracle as O
from test_tpcc_carry import host_carry, host_concat, host_take

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import tpcc as T  # noqa: E402

ORACLE_CC = {dvcc.NO_WAIT: O.NO_WAIT, dvcc.WAIT_DIE: O.WAIT_DIE, dvcc.OCC: O.OCC}
CCS = [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC]
MAX_TXN_ACC = 33  # NewOrder with 15 lines: 3 + 2 * 15


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


def _params(num_wh=8, **kw):
    d = dict(num_wh=num_wh, cust_per_dist=1000, max_items=2000)
    d.update(kw)
    return O.tpcc_params(**d), T.tpcc_params(**d)


def _check_tables(eng, db):
    for t in range(5):
        ref = db.table(t)
        for col in range(3):
            got = eng.read_col(t, col)
            assert (got == ref[1 + col]).all(), f"table {t} col {col}: {np.flatnonzero(got != ref[1 + col])[:5]}"


def _ref(db, cc, e):
    c, o, st = db.epoch(ORACLE_CC[cc], e.keys, e.types, e.tables, e.args, e.txn_begin)
    return c.copy(), o.copy(), st


def _same_epoch(dep, d_args, host, what=""):
    """a device epoch's five arrays against the host's"""
    assert (dep.n_txn, dep.n_acc) == (host.n_txn, host.n_acc), what
    assert np.array_equal(dep.keys.cpu().numpy().view(np.uint64), host.keys), what
    assert np.array_equal(dep.types.cpu().numpy(), host.types), what
    assert np.array_equal(dep.tables.cpu().numpy(), host.tables), what
    assert np.array_equal(d_args.cpu().numpy().view(np.uint64), host.args), what
    assert np.array_equal(dep.acc_txn.cpu().numpy().view(np.uint32), host.acc_txn()), what  # = txn_begin


def _same_outcome(k, c, o, st, c_ref, o_ref, st_ref, host):
    assert np.array_equal(c[:host.n_txn], c_ref), f"epoch {k}: commit bytes at {np.flatnonzero(c[:host.n_txn] != c_ref)[:5]}"
    assert np.array_equal(o[:host.n_txn], o_ref), f"epoch {k}: o_id at {np.flatnonzero(o[:host.n_txn] != o_ref)[:5]}"
    assert (st.n_txn, st.n_acc, st.committed, st.write_cnt) == (host.n_txn, host.n_acc, st_ref.committed,
                                                               st_ref.write_cnt), k


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("n,perc", [(1000, 0.5), (512, 1.0), (512, 0.0)])
def test_tpcc_carry(cc, n, perc):
    """A host-driven closed loop of fixed-size epochs: dv_tpcc_epoch_carry
    after every epoch against host_carry, the cap alternately above and
    inside the aborted set; 1,000 txns of 3..33 accesses span four carry
    blocks, perc 1.0 / 0.0 make every txn 3 accesses / a NewOrder"""
    po, pp = _params(perc_payment=perc)
    db = O.TpccDB(po, 5)
    eng = T.TpccEngine(cc, pp, n, seed=5)
    try:
        host = T.gen(pp, n, 700)
        dep, d_args = T.device_epoch(host)
        d_commit = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_oid = torch.zeros(n, dtype=torch.int64, device="cuda")
        carried = 0
        for k in range(5):
            c_ref, o_ref, st_ref = _ref(db, cc, host)
            st = eng.run_tpcc_epoch_device(dep, d_args, d_commit, d_oid)
            _same_outcome(k, d_commit.cpu().numpy(), d_oid.cpu().numpy().view(np.uint64), st, c_ref, o_ref, st_ref,
                          host)
            cap = n if k % 2 == 0 else n // 3
            hc = host_carry(host, c_ref, cap)
            assert k % 2 == 0 or int((c_ref == 0).sum()) > cap, "the cap does not cut inside the aborted set"
            dc, dc_args = eng.carry(dep, d_args, cap)
            _same_epoch(dc, dc_args, hc, f"carry of epoch {k}")
            assert dc.max_txn_acc == dep.max_txn_acc
            carried += hc.n_txn
            assert hc.n_txn < n
            new = T.gen(pp, n - hc.n_txn, 701 + k)
            host = host_concat(hc, new)
            dnew, dnew_args = T.device_epoch(new)
            dep = dvcc.DeviceEpoch.concat(dc, dnew)
            d_args = torch.cat([dc_args, dnew_args])
        assert carried > 0
        _check_tables(eng, db)
    finally:
        eng.close()


def test_tpcc_carry_edges():
    po, pp = _params(num_wh=2)
    one = T.gen(pp, 1, 5)  # (a NewOrder of 33 accesses)
    assert _ref(O.TpccDB(po, 5), dvcc.NO_WAIT, one)[0][0] == 1
    eng = T.TpccEngine(dvcc.NO_WAIT, pp, 400, seed=5)
    try:
        dep, d_args = T.device_epoch(one)
        eng.run_tpcc_epoch_device(dep, d_args, torch.zeros(1, dtype=torch.uint8, device="cuda"))
        dc, dc_args = eng.carry(dep, d_args)  # its only txn commits: nothing to carry
        assert (dc.n_txn, dc.n_acc, dc_args.numel()) == (0, 0, 0)
        e = T.gen(pp, 200, 4)
        dep, d_args = T.device_epoch(e)
        eng.run_tpcc_epoch_device(dep, d_args, torch.zeros(200, dtype=torch.uint8, device="cuda"))
        other, other_args = T.device_epoch(T.gen(pp, 100, 5))
        with pytest.raises(dvcc.DvccError) as ei:  # not the epoch the context decided last
            eng.carry(other, other_args)
        assert ei.value.code == dvcc._lib.DV_ERR_STATE
        with pytest.raises(dvcc.DvccError):  # ... nor are the same sizes in other buffers
            eng.carry(*T.device_epoch(e))
        dc, _ = eng.carry(dep, d_args)  # (the decided one still carries)
        assert dc.n_txn > 0
    finally:
        eng.close()
    eng = T.TpccEngine(dvcc.CALVIN, pp, 400, seed=5)
    try:
        eng.run_tpcc_epoch_device(dep, d_args, torch.zeros(200, dtype=torch.uint8, device="cuda"))
        with pytest.raises(dvcc.DvccError) as ei:  # CALVIN never aborts
            eng.carry(dep, d_args)
        assert ei.value.code == dvcc._lib.DV_ERR_STATE
    finally:
        eng.close()


# ---- the device closed loop ------------------------------------------------
# a pool of 560 read from txn 540: the first take (512 txns) wraps, and so few
# txns commit per epoch (8..41) that the cursor then creeps from 492 to the
# pool's end -- NO_WAIT / WAIT_DIE cross it in the refill behind epoch 1, OCC
# in the one behind epoch 5 (_loop_ref asserts both wraps)
N_LOOP, POOL, CUR0, EPOCHS = 512, 560, 540, 8

_loop_cache = {}


def _loop_ref(cc):
    """the oracle's closed loop (computed once per CC, read-only afterwards):
    per-epoch (commit, o_id, stats, epoch), the epoch left, the cursor and the
    final tables"""
    if cc in _loop_cache:
        return _loop_cache[cc]
    po, pp = _params()
    db = O.TpccDB(po, 5)
    pool = T.gen(pp, POOL, 900)
    cur = CUR0
    host = host_take(pool, cur, N_LOOP)
    wraps = [cur + N_LOOP > pool.n_txn]
    cur = (cur + N_LOOP) % pool.n_txn
    out = []
    for _ in range(EPOCHS):
        c_ref, o_ref, st_ref = _ref(db, cc, host)
        out.append((c_ref, o_ref, st_ref, host))
        hc = host_carry(host, c_ref, N_LOOP)
        fresh = N_LOOP - hc.n_txn
        wraps.append(cur + fresh > pool.n_txn)
        host = host_concat(hc, host_take(pool, cur, fresh))
        cur = (cur + fresh) % pool.n_txn
    # the shape must keep exercising the wrap-around of the pool: in the first
    # take, and in a refill whose epoch the loop then runs
    assert wraps[0], "the first take does not wrap"
    assert any(wraps[1:EPOCHS]), f"no later refill wraps (cc {cc})"
    tables = [db.table(t) for t in range(5)]
    _loop_cache[cc] = (pp, pool, out, host, cur, tables)
    return _loop_cache[cc]


def _run_loop(cc, splits, limits=None):
    pp, pool, ref, nxt, cur_ref, tables = _loop_ref(cc)
    eng = T.TpccEngine(cc, pp, N_LOOP, seed=5)
    if limits:
        eng.set_async_limits(*limits)
    try:
        dpool, pargs = T.device_epoch(pool)
        assert dpool.max_txn_acc <= MAX_TXN_ACC
        dpool.max_txn_acc = MAX_TXN_ACC
        pb = torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()
        cursor = torch.full((1,), CUR0, dtype=torch.int32, device="cuda")
        bufs, got = None, []
        for call, n_ep in enumerate(splits):
            commits = [torch.zeros(N_LOOP, dtype=torch.uint8, device="cuda") for _ in range(n_ep)]
            oids = [torch.zeros(N_LOOP, dtype=torch.int64, device="cuda") for _ in range(n_ep)]
            sts, bufs, cursor = eng.closed_loop(dpool, pargs, pb, N_LOOP, n_ep, cursor=cursor, bufs=bufs,
                                                d_commits=commits, d_oids=oids, resume=call > 0)
            got += [(c.cpu().numpy(), o.cpu().numpy().view(np.uint64), s) for c, o, s in zip(commits, oids, sts)]
            if n_ep & 1:
                bufs.swap()
        assert len(got) == EPOCHS
        for k, ((c, o, st), (c_ref, o_ref, st_ref, host)) in enumerate(zip(got, ref)):
            _same_outcome(k, c, o, st, c_ref, o_ref, st_ref, host)
        assert int(cursor.item()) == cur_ref
        e, e_args = bufs.epoch(0, N_LOOP, MAX_TXN_ACC)
        _same_epoch(e, e_args, nxt, "the epoch left in the buffers")
        for t in range(5):
            for col in range(3):
                assert (eng.read_col(t, col) == tables[t][1 + col]).all(), f"table {t} col {col}"
        return [st for _, _, st in got]
    finally:
        eng.close()


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("splits", [(8,), (4, 4), (3, 5)])
def test_tpcc_device_closed_loop(cc, splits):
    """dv_tpcc_epoch_run_closed_loop against the oracle's host loop, the pool
    wrapping in the first take and in a later refill: one call, two calls of
    4 with resume, and 3 + 5 (odd counts: the buffers -- args too -- swap)"""
    _run_loop(cc, splits)


@pytest.mark.parametrize("cc", CCS)
def test_tpcc_device_closed_loop_halts(cc):
    """asynchronous decision launches forced to yield: every such epoch is
    decided again synchronously before its successor is rebuilt"""
    sts = _run_loop(cc, (8,), limits=(1, 1))
    print("async_yields per epoch:", [st.async_yields for st in sts])
    assert sum(st.async_yields for st in sts) > 0, "no asynchronous launch yielded"


def test_tpcc_closed_loop_args():
    po, pp = _params(num_wh=2)
    pool = T.gen(pp, 300, 13)
    dpool, pargs = T.device_epoch(pool)
    dpool.max_txn_acc = MAX_TXN_ACC
    pb = torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()
    eng = T.TpccEngine(dvcc.NO_WAIT, pp, 400, seed=5)
    try:
        before = [eng.read_col(t, c) for t in range(5) for c in range(3)]
        with pytest.raises(dvcc.DvccError):  # more txns per epoch than the pool holds
            eng.closed_loop(dpool, pargs, pb, 301, 2)
        with pytest.raises(dvcc.DvccError):  # buffers below an epoch's bound
            eng.closed_loop(dpool, pargs, pb, 200, 2, bufs=T.TpccLoopBufs(200 * MAX_TXN_ACC - 1, "cuda"))
        with pytest.raises(dvcc.DvccError):  # no buffers for the operation words
            eng.closed_loop(dpool, pargs, pb, 200, 2, bufs=dvcc.ClosedLoopBufs(200 * MAX_TXN_ACC, True, "cuda"))
        with pytest.raises(dvcc.DvccError):  # ... nor the pool's
            eng.closed_loop(dpool, None, pb, 200, 2)
        after = [eng.read_col(t, c) for t in range(5) for c in range(3)]
        assert all((a == b).all() for a, b in zip(after, before)), "a rejected call ran something"
        eng.closed_loop(dpool, pargs, pb, 200, 2)
    finally:
        eng.close()
    eng = T.TpccEngine(dvcc.CALVIN, pp, 400, seed=5)
    try:
        with pytest.raises(dvcc.DvccError):  # no aborts to carry
            eng.closed_loop(dpool, pargs, pb, 200, 2)
    finally:
        eng.close()
    ycsb = dvcc.CCEngine(dvcc.NO_WAIT, 400, 400 * MAX_TXN_ACC)
    try:
        ycsb.load_ycsb_partition(1 << 10)
        with pytest.raises(dvcc.DvccError):  # a YCSB context
            T.TpccEngine.closed_loop(ycsb, dpool, pargs, pb, 200, 2)
    finally:
        ycsb.close()


@pytest.mark.parametrize("cc", CCS)
def test_tpcc_n_acc_dev(cc):
    """One TPC-C epoch with its exact n_acc, and with n_acc a padded bound --
    the real count in a device word, garbage in every array past it: the same
    commit bytes, o_id, stats and tables as the oracle either way"""
    n = 1000
    po, pp = _params(num_wh=4)
    e = T.gen(pp, n, 31)
    c_ref, o_ref, st_ref = _ref(O.TpccDB(po, 5), cc, e)
    bound = n * MAX_TXN_ACC
    assert e.n_acc < bound
    rng = np.random.default_rng(7)
    for padded in (False, True):
        db = O.TpccDB(po, 5)
        _ref(db, cc, e)
        eng = T.TpccEngine(cc, pp, n, seed=5)
        try:
            dep, d_args = T.device_epoch(e)
            if padded:
                def pad(t, junk):
                    return torch.cat([t, torch.from_numpy(junk).to(t.device).view(t.dtype)])
                g = bound - e.n_acc
                dep = dvcc.DeviceEpoch.from_tensors(
                    pad(dep.keys, rng.integers(0, 1 << 62, g, dtype=np.int64)),
                    pad(dep.types, rng.integers(0, 255, g, dtype=np.uint8)),
                    pad(dep.acc_txn, rng.integers(0, 1 << 31, g, dtype=np.int32)), n,
                    tables=pad(dep.tables, rng.integers(0, 255, g, dtype=np.uint8)), max_txn_acc=MAX_TXN_ACC)
                d_args = pad(d_args, rng.integers(0, 1 << 62, g, dtype=np.int64))
                dep.n_acc_dev = torch.tensor([e.n_acc], dtype=torch.int32, device="cuda")
                assert dep.n_acc == bound
            d_commit = torch.zeros(n, dtype=torch.uint8, device="cuda")
            d_oid = torch.zeros(n, dtype=torch.int64, device="cuda")
            st = eng.run_tpcc_epoch_device(dep, d_args, d_commit, d_oid)
            _same_outcome(int(padded), d_commit.cpu().numpy(), d_oid.cpu().numpy().view(np.uint64), st, c_ref, o_ref,
                          st_ref, e)
            _check_tables(eng, db)
        finally:
            eng.close()


def test_tpcc_n_acc_dev_calvin_rejected():
    po, pp = _params(num_wh=2)
    e = T.gen(pp, 64, 32)
    eng = T.TpccEngine(dvcc.CALVIN, pp, 64, seed=5)
    try:
        dep, d_args = T.device_epoch(e)
        dep.n_acc_dev = torch.tensor([e.n_acc], dtype=torch.int32, device="cuda")
        with pytest.raises(dvcc.DvccError) as ei:
            eng.run_tpcc_epoch_device(dep, d_args, torch.zeros(64, dtype=torch.uint8, device="cuda"))
        assert ei.value.code == dvcc._lib.DV_ERR_ARG
    finally:
        eng.close()
