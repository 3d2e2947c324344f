"""Exponential back-off in the TPC-C closed loop (dv_tpcc_closed_loop_backoff):
the reference -- tests/test_loop_backoff.py's BackoffModel, which knows nothing
of the workload, driven by the oracle's TpccDB.epoch -- and the CPU checks:
that the shapes the GPU tests run exercise what they are meant to, the model
at D = 1 against the host loop of host_carry / host_take / host_concat,
conservation, the slot bound, and the entry point itself.

The epoch of a model state (src, born, aborts) is test_tpcc_carry._select(pool,
src): a released txn's accesses are read from the pool again with their table
bytes and operation words.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import _oracle as O
import dvcc
from dvcc import _lib as L
from dvcc import tpcc as T
from test_loop_backoff import BackoffModel, _desc, check_conservation, malformed_descs, slot_bound
from test_tpcc_carry import _select, host_carry, host_concat, host_take

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_CC = {dvcc.NO_WAIT: O.NO_WAIT, dvcc.WAIT_DIE: O.WAIT_DIE, dvcc.OCC: O.OCC}
CCS = [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC]
DB_SEED = 5

# name: (tpcc_params overrides, pool txns, pool seed, first cursor, txns per epoch, epochs)
SHAPES = {
    # 512 txns: two gather blocks; a pool of 800 read from 780: the first take wraps
    "main": (dict(num_wh=8), 800, 900, 780, 512, 24),
    # every txn a Payment on the one warehouse: each epoch commits exactly its first txn
    "closed form": (dict(num_wh=1, perc_payment=1.0), 600, 900, 0, 256, 12),
    # 1,000 txns: four carry blocks, the last ragged
    "four blocks": (dict(num_wh=8), 3000, 900, 2900, 1000, 12),
    # the shape of the commit counts quoted in DESIGN 5b
    "payment half": (dict(num_wh=8, perc_payment=0.5), 3000, 900, 2900, 512, 24),
}


def params(**kw):
    """(oracle params, dvcc params), as tests/test_tpcc_closed_loop.py's _params"""
    d = dict(num_wh=8, cust_per_dist=1000, max_items=2000)
    d.update(kw)
    return O.tpcc_params(**d), T.tpcc_params(**d)


def _wraps(words):
    """a run of fresh identity words passes the pool's end"""
    return bool((np.diff(words & 0xFFFFFFFF) < 0).any())


def host_tpcc_backoff_loop(cc, po, pool, cur, n_txn, n_epochs, D, **kw):
    """the oracle's TPC-C loop under the model: per epoch (commit bytes, o_id,
    stats, the host epoch), the epoch left, the model, the final tables and
    the largest abort count ever parked"""
    db = O.TpccDB(po, DB_SEED)
    m = BackoffModel(pool.n_txn, cur, n_txn, D, **kw)
    host = _select(pool, m.build()[0])
    out, most = [], 0
    for _ in range(n_epochs):
        c, o, st = db.epoch(ORACLE_CC[cc], host.keys, host.types, host.tables, host.args, host.txn_begin)
        out.append((c[:host.n_txn].copy(), o[:host.n_txn].copy(), st, host))
        host = _select(pool, m.epoch(c)[0])
        most = max([most] + [int(s[2].max()) for s in m.slots if len(s[2])])
    return out, host, m, [db.table(t) for t in range(5)], most


_cache = {}


def ref_tpcc_backoff(cc, shape, D, epochs=None, **kw):
    """computed once per case, read-only afterwards: dict(pp, pool, ref, nxt,
    model, tables, most, n, epochs, cur0); epochs: fewer than the shape's (the
    state between two calls)"""
    key = (cc, shape, D, epochs, tuple(sorted(kw.items())))
    if key not in _cache:
        over, pool_n, pool_seed, cur0, n, shape_epochs = SHAPES[shape]
        epochs = shape_epochs if epochs is None else epochs
        po, pp = params(**over)
        if ("pool", shape) not in _cache:
            _cache[("pool", shape)] = T.gen(pp, pool_n, pool_seed)
        pool = _cache[("pool", shape)]
        ref, nxt, m, tables, most = host_tpcc_backoff_loop(cc, po, pool, cur0, n, epochs, D, **kw)
        _cache[key] = dict(pp=pp, pool=pool, ref=ref, nxt=nxt, model=m, tables=tables, most=most, n=n, epochs=epochs,
                           cur0=cur0)
    return _cache[key]


@pytest.mark.parametrize("cc", CCS)
def test_the_main_shape_qualifies(cc):
    """what the GPU test of the main shape relies on, shown by the model"""
    most = {}
    for D in (1, 2, 4, 8, 16):
        r = ref_tpcc_backoff(cc, "main", D)
        m, E = r["model"], r["epochs"]
        assert _wraps(m.drawn[0]), f"D {D}: the first take does not wrap"
        assert any(_wraps(w) for w in m.drawn[1:E]), f"D {D}: no later refill wraps"
        assert m.lost == 0 and m.fullest <= slot_bound(r["n"], D)
        assert (m.spilled > 0) == (D >= 2), f"D {D}: spill {m.spilled}"
        assert 0 < m.totals[0] < r["n"] * E
        most[D] = r["most"]
    print("cc", cc, "largest abort count parked per D:", most)
    assert most[16] >= 5, "no fifth abort parked at D = 16 (class 4)"


@pytest.mark.parametrize("cc", CCS)
def test_d1_is_the_host_loop(cc):
    """the model at D = 1 against host_carry / host_take / host_concat around
    the oracle: the epochs' five arrays, commit bytes, cursor"""
    r = ref_tpcc_backoff(cc, "main", 1)
    pool, n, E = r["pool"], r["n"], r["epochs"]
    db = O.TpccDB(params(**SHAPES["main"][0])[0], DB_SEED)
    cur = r["cur0"]
    host = host_take(pool, cur, n)
    cur = (cur + n) % pool.n_txn
    for k in range(E + 1):
        h = r["ref"][k][3] if k < E else r["nxt"]
        for name in ("keys", "types", "tables", "args", "txn_begin"):
            assert np.array_equal(getattr(h, name), getattr(host, name)), f"epoch {k}: {name}"
        if k == E:
            break
        c, _, st = db.epoch(ORACLE_CC[cc], host.keys, host.types, host.tables, host.args, host.txn_begin)
        assert np.array_equal(c[:n], r["ref"][k][0]) and st.committed == r["ref"][k][2].committed, k
        hc = host_carry(host, c, n)
        host = host_concat(hc, host_take(pool, cur, n - hc.n_txn))
        cur = (cur + n - hc.n_txn) % pool.n_txn
    m = r["model"]
    assert m.cur == cur and m.spilled == 0 and m.lost == 0
    assert m.totals[0] == sum(x[2].committed for x in r["ref"])


@pytest.mark.parametrize("shape,Ds", [("main", (1, 2, 4, 8, 16)), ("closed form", (2, 8)), ("four blocks", (4,))])
def test_conservation_and_the_slot_bound(shape, Ds):
    for cc in CCS:
        for D in Ds:
            r = ref_tpcc_backoff(cc, shape, D)
            m = r["model"]
            check_conservation(m)
            assert m.lost == 0 and m.fullest <= slot_bound(r["n"], D)
            assert m.totals[0] + m.totals[1] == r["n"] * r["epochs"] and m.epoch_end[-1] == m.totals[0]


def test_the_closed_form_commits_one_txn_per_epoch():
    for cc in CCS:
        for D, spill in ((2, 258), (8, 1483)):
            r = ref_tpcc_backoff(cc, "closed form", D)
            assert all(int(c.sum()) == 1 and c[0] == 1 for c, _, _, _ in r["ref"]), (cc, D)
            assert r["model"].spilled == spill


def test_a_small_slot_cap_loses_entries():
    full = ref_tpcc_backoff(dvcc.NO_WAIT, "four blocks", 4)["model"]
    assert full.lost == 0 and full.fullest > 1100
    m = ref_tpcc_backoff(dvcc.NO_WAIT, "four blocks", 4, slot_cap=1100)["model"]
    assert m.lost == 3720 and m.fullest == 1100


def test_backing_off_commits_more_under_2pl():
    """the scheduling effect, a property of the rule: commits in 24 epochs of
    512 txns at 8 warehouses, half Payments"""
    got = {(cc, D): ref_tpcc_backoff(cc, "payment half", D)["model"].totals[0]
           for cc in CCS for D in (1, 8)}
    print(got)
    for cc in (dvcc.NO_WAIT, dvcc.WAIT_DIE):
        assert (got[cc, 1], got[cc, 8]) == (398, 684)
    assert (got[dvcc.OCC, 1], got[dvcc.OCC, 8]) == (366, 382)


def test_the_header_declares_the_entry_and_it_refuses_a_null_context():
    with open(os.path.join(ROOT, "include", "dvcc.h")) as f:
        text = f.read()
    assert re.search(r"int\s+dv_tpcc_closed_loop_backoff\(dv_ctx \*ctx, const dv_loop_backoff \*bo\);", text)
    assert ("dv_tpcc_closed_loop_backoff", ctypes.c_int,
            [ctypes.c_void_p, ctypes.POINTER(L.LoopBackoffDesc)]) in L.SIGNATURES
    f = L.lib().dv_tpcc_closed_loop_backoff
    assert f(None, None) == L.DV_ERR_ARG
    assert f(None, ctypes.byref(_desc())) == L.DV_ERR_ARG
    for name, d in malformed_descs():
        assert f(None, ctypes.byref(d)) == L.DV_ERR_ARG, name
    assert dvcc.TpccLoopBackoff is T.TpccLoopBackoff and issubclass(T.TpccLoopBackoff, dvcc.LoopBackoff)
