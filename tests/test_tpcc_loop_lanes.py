"""The TPC-C closed loop over decision lanes, with tracker and back-off
(dv_tpcc_epoch_run_closed_loop_lanes, dv_tpcc_closed_loop_backoff_lanes): the
reference -- tests/test_loop_backoff_lanes.py's LanesBackoffModel, which knows
nothing of the workload, driven by the oracle's TpccDB.epoch over
test_tpcc_carry._select(pool, src) -- and the CPU checks: that the shapes the
GPU tests run exercise what they are meant to, a few pinned figures, the model
at L = 1 against the single loop's reference and at D = 1 against a plain host
lanes loop of host_carry / host_take / host_concat, conservation, the header
and the entry points.  The model is never driven by the engine.

One sequence of epochs: epoch k + L is built after epoch k is decided, from
slot (k + L) % D and then the pool at the one cursor, so the epochs, commit
bytes, o_ids and tables are those of a single worker running epoch 0, 1, 2, ..
in which an abort of epoch k returns in epoch k + L at the earliest.
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
from test_loop_backoff import _desc, check_conservation, malformed_descs, slot_bound
from test_loop_backoff_lanes import MAX_LANES, LanesBackoffModel
from test_tpcc_carry import _select, host_carry, host_concat, host_take
from test_tpcc_loop_backoff import CCS, DB_SEED, ORACLE_CC, SHAPES, _wraps, params, ref_tpcc_backoff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = (2, 3, 4)
# An epoch's access bound above the 2,097,152 accesses up to which an epoch's
# decision is queued as round 0 and one asynchronous launch on its own (the
# lanes loop queues that form whatever the bound): 16,400 txns declared at the
# longest txn the engine takes, 128 accesses -- config E's case (65,536 x 33)
# at a quarter of its txns.  The first take wraps the pool.
WIDE, WIDE_ACC = "wide bound", 128
SHAPES = dict(SHAPES, **{WIDE: (dict(num_wh=8), 20000, 900, 15000, 16400, 12)})


def host_tpcc_lanes_loop(cc, po, pool, cur, n_txn, n_epochs, D, lanes, **kw):
    """the oracle's TPC-C loop under the lanes model: per epoch (commit bytes,
    o_id, stats, the host epoch), the L epochs left (by number), the model and
    the final tables"""
    db = O.TpccDB(po, DB_SEED)
    m = LanesBackoffModel(pool.n_txn, cur, n_txn, D, lanes, **kw)
    hosts = {e: _select(pool, ep[0]) for e, ep in enumerate(m.start())}
    out = []
    for k in range(n_epochs):
        host = hosts.pop(k)
        c, o, st = db.epoch(ORACLE_CC[cc], host.keys, host.types, host.tables, host.args, host.txn_begin)
        out.append((c[:host.n_txn].copy(), o[:host.n_txn].copy(), st, host))
        hosts[k + lanes] = _select(pool, m.epoch(c)[0])
    return out, hosts, m, [db.table(t) for t in range(5)]


_cache = {}


def ref_tpcc_lanes(cc, shape, D, lanes, epochs=None, **kw):
    """computed once per case, read-only afterwards: dict(pp, pool, ref, nxt
    (epoch number -> host epoch), model, tables, n, epochs, cur0); epochs
    defaults to 6 L"""
    epochs = 6 * lanes if epochs is None else epochs
    key = (cc, shape, D, lanes, epochs, tuple(sorted(kw.items())))
    if key not in _cache:
        over, pool_n, pool_seed, cur0, n, _ = SHAPES[shape]
        po, pp = params(**over)
        if ("pool", shape) not in _cache:
            _cache[("pool", shape)] = T.gen(pp, pool_n, pool_seed)
        pool = _cache[("pool", shape)]
        ref, nxt, m, tables = host_tpcc_lanes_loop(cc, po, pool, cur0, n, epochs, D, lanes, **kw)
        _cache[key] = dict(pp=pp, pool=pool, ref=ref, nxt=nxt, model=m, tables=tables, n=n, epochs=epochs, cur0=cur0)
    return _cache[key]


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("lanes", LANES)
def test_the_main_shape_qualifies(cc, lanes):
    """what the GPU tests of the main shape rely on, shown by the model"""
    for D in (1, 2, 4, 8):
        r = ref_tpcc_lanes(cc, "main", D, lanes)
        m, E, n = r["model"], r["epochs"], r["n"]
        assert len(m.drawn) == E + lanes
        assert any(_wraps(w) for w in m.drawn[:lanes]), f"D {D}: no take among the first L wraps"
        if D >= 2:  # (at D = 1 this fails for L = 2 and for OCC at L = 4)
            assert any(_wraps(w) for w in m.drawn[lanes:]), f"D {D}: no later refill wraps"
        assert (m.spilled > 0) == (D >= 2), f"D {D}: spill {m.spilled}"
        assert m.lost == 0 and m.fullest <= slot_bound(n, D)
        assert m.classes >= set(range(min(m.lgD, 3) + 1)), f"D {D}: classes {m.classes}"
        assert m.totals[3] >= 3, f"D {D}: no txn commits at its third retry"
        assert m.totals[0] + m.totals[1] == n * E and m.epoch_end[-1] == m.totals[0]


def _closed_form_holds(r):
    return all(int(c.sum()) == 1 and c[0] == 1 for c, _, _, _ in r["ref"])


def test_pinned_figures():
    r = ref_tpcc_lanes(dvcc.NO_WAIT, "main", 2, 2)
    assert (r["epochs"], r["model"].totals[0], r["model"].spilled) == (12, 290, 491)
    r = ref_tpcc_lanes(dvcc.NO_WAIT, "main", 8, 4)
    assert (r["epochs"], r["model"].totals[0]) == (24, 633)
    for cc in CCS:  # (every epoch commits exactly its first txn, whatever the CC)
        for lanes, D, spill in ((2, 2, 256), (2, 4, 2256), (4, 4, 3051)):
            r = ref_tpcc_lanes(cc, "closed form", D, lanes)
            assert _closed_form_holds(r), (cc, lanes, D)
            assert r["model"].spilled == spill and r["model"].lost == 0, (cc, lanes, D, r["model"].spilled)


def test_the_wide_bound_shape_qualifies():
    r = ref_tpcc_lanes(dvcc.WAIT_DIE, WIDE, 4, 2)
    m, n = r["model"], r["n"]
    assert r["epochs"] == 12 and n * WIDE_ACC > 2 << 20 >= n * 33
    assert all(h.n_acc < 2 << 20 for _, _, _, h in r["ref"])
    assert _wraps(m.drawn[0]) and any(_wraps(w) for w in m.drawn[2:])
    assert m.spilled > 0 and m.lost == 0 and m.totals[3] >= 3 and m.classes == {0, 1, 2}
    check_conservation(m)


def test_a_small_slot_cap_loses_entries():
    full = ref_tpcc_lanes(dvcc.NO_WAIT, "four blocks", 4, 2)["model"]
    assert full.lost == 0 and full.fullest > 1100 and full.spilled > 0
    m = ref_tpcc_lanes(dvcc.NO_WAIT, "four blocks", 4, 2, slot_cap=1100)["model"]
    assert (m.lost, m.fullest) == (1597, 1100)


def test_one_lane_is_the_single_loop():
    """the model at L = 1 against ref_tpcc_backoff: epochs, commit bytes,
    o_ids, the ring, the log, the counters, the tables"""
    cc, D = dvcc.WAIT_DIE, 4
    one = ref_tpcc_backoff(cc, "main", D)
    r = ref_tpcc_lanes(cc, "main", D, 1, epochs=one["epochs"])
    m, s = r["model"], one["model"]
    for k, ((c, o, _, h), (sc, so, _, sh)) in enumerate(zip(r["ref"], one["ref"])):
        assert np.array_equal(c, sc) and np.array_equal(o, so), k
        for name in ("keys", "types", "tables", "args", "txn_begin"):
            assert np.array_equal(getattr(h, name), getattr(sh, name)), f"epoch {k}: {name}"
    E = r["epochs"]
    assert list(r["nxt"]) == [E] and np.array_equal(r["nxt"][E].keys, one["nxt"].keys)
    assert m.cur == s.cur and m.counters() == s.counters() and m.totals == s.totals
    assert m.epoch_end == s.epoch_end and np.array_equal(m.hist, s.hist)
    assert np.array_equal(m.log_words(), s.log_words())
    for a, b in zip(m.slots, s.slots):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for t in range(5):
        for col in range(4):
            assert np.array_equal(r["tables"][t][col], one["tables"][t][col])


@pytest.mark.parametrize("cc", CCS)
@pytest.mark.parametrize("lanes", LANES)
def test_d1_is_the_plain_host_lanes_loop(cc, lanes):
    """the model at D = 1 against host_carry / host_take / host_concat around
    the oracle with one shared cursor: the epochs' five arrays, commit bytes,
    the L epochs left, the cursor"""
    r = ref_tpcc_lanes(cc, "main", 1, lanes)
    pool, n, E = r["pool"], r["n"], r["epochs"]
    db = O.TpccDB(params(**SHAPES["main"][0])[0], DB_SEED)
    cur, hosts = r["cur0"], {}
    for ln in range(lanes):
        hosts[ln] = host_take(pool, cur, n)
        cur = (cur + n) % pool.n_txn

    def same(h, host, k):
        for name in ("keys", "types", "tables", "args", "txn_begin"):
            assert np.array_equal(getattr(h, name), getattr(host, name)), f"epoch {k}: {name}"

    for k in range(E):
        host = hosts.pop(k)
        same(r["ref"][k][3], host, k)
        c, o, st = db.epoch(ORACLE_CC[cc], host.keys, host.types, host.tables, host.args, host.txn_begin)
        assert np.array_equal(c[:n], r["ref"][k][0]) and np.array_equal(o[:n], r["ref"][k][1]), k
        hc = host_carry(host, c, n)
        hosts[k + lanes] = host_concat(hc, host_take(pool, cur, n - hc.n_txn))
        cur = (cur + n - hc.n_txn) % pool.n_txn
    assert sorted(hosts) == sorted(r["nxt"]) == list(range(E, E + lanes))
    for e in hosts:
        same(r["nxt"][e], hosts[e], e)
    m = r["model"]
    assert m.cur == cur and m.spilled == 0 and m.lost == 0
    assert m.totals[0] == sum(x[2].committed for x in r["ref"])
    for e in r["nxt"]:  # an abort per L epochs
        assert np.array_equal(m.aborts_of(e) * lanes, e - (m.words(e) >> 32))


@pytest.mark.parametrize("shape,cases", [("main", [(L_, D) for L_ in LANES for D in (1, 2, 4, 8)]),
                                         ("closed form", [(2, 2), (2, 4), (4, 4)]), ("four blocks", [(2, 4)])])
def test_conservation_and_the_slot_bound(shape, cases):
    for cc in CCS:
        for lanes, D in cases:
            r = ref_tpcc_lanes(cc, shape, D, lanes)
            m = r["model"]
            check_conservation(m)
            assert m.lost == 0 and m.fullest <= slot_bound(r["n"], D)
            assert m.totals[0] + m.totals[1] == r["n"] * r["epochs"] and m.epoch_end[-1] == m.totals[0]
            for e, (src, born, ab) in m.eps.items():  # a txn with a aborts has waited a L epochs at least
                assert (e - born >= ab * lanes).all()


def test_the_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "dvcc.h")).read()
    s = r"\s*"
    assert re.search(
        r"int\s+dv_tpcc_epoch_run_closed_loop_lanes\s*\(\s*dv_ctx\s*\*\s*const\s*\*\s*lanes\s*,"
        r"\s*uint32_t\s+n_lanes\s*,"
        r"\s*const\s+dv_epoch_dev\s*\*\s*pool\s*,\s*const\s+uint64_t\s*\*\s*pool_args\s*,\s*const\s+uint32_t\s*\*"
        r"\s*pool_begin\s*,\s*uint32_t\s*\*\s*cursor\s*,\s*uint32_t\s+n_txn\s*,\s*dv_epoch_dev\s*\*\s*bufs\s*,"
        r"\s*uint64_t\s*\*\s*const\s*\*\s*buf_args\s*,\s*uint64_t\s+buf_cap\s*,\s*uint32_t\s+n_epochs\s*,"
        r"\s*int\s+resume\s*,\s*uint8_t\s*\*\s*const\s*\*\s*d_commits\s*,\s*uint64_t\s*\*\s*const\s*\*\s*d_oids\s*,"
        r"\s*dv_stats\s*\*\s*sts\s*\)\s*;", text)
    assert re.search(r"int\s+dv_tpcc_closed_loop_backoff_lanes" + s + r"\(" + s + r"dv_ctx" + s + r"\*" + s + r"ctx"
                     + s + r"," + s + r"const\s+dv_loop_backoff" + s + r"\*" + s + r"bo" + s + r"," + s
                     + r"uint32_t\s+n_lanes" + s + r"\)" + s + r";", text)
    vp, P = ctypes.c_void_p, ctypes.POINTER
    assert ("dv_tpcc_epoch_run_closed_loop_lanes", ctypes.c_int,
            [P(vp), ctypes.c_uint32, P(L.EpochDev), vp, vp, vp, ctypes.c_uint32, P(L.EpochDev), P(vp),
             ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, P(vp), P(vp), P(L.Stats)]) in L.SIGNATURES
    assert ("dv_tpcc_closed_loop_backoff_lanes", ctypes.c_int,
            [vp, P(L.LoopBackoffDesc), ctypes.c_uint32]) in L.SIGNATURES
    assert callable(T.TpccEngine.closed_loop_lanes)


def test_the_entries_refuse_null_contexts_and_malformed_descriptors():
    f = L.lib().dv_tpcc_closed_loop_backoff_lanes
    for n_lanes in (0, 1, 2, MAX_LANES, MAX_LANES + 1):
        assert f(None, None, n_lanes) == L.DV_ERR_ARG
        assert f(None, ctypes.byref(_desc()), n_lanes) == L.DV_ERR_ARG
    for name, d in malformed_descs():
        assert f(None, ctypes.byref(d), 2) == L.DV_ERR_ARG, name
    g = L.lib().dv_tpcc_epoch_run_closed_loop_lanes
    word = (ctypes.c_uint32 * 2)()
    one = (ctypes.c_void_p * 2)(None, None)
    pool, bufs = L.EpochDev(), (L.EpochDev * 4)()
    for lanes, n_lanes in ((None, 2), (one, 0), (one, 2), (one, MAX_LANES + 1), (one, 1)):
        assert g(lanes, n_lanes, ctypes.byref(pool), ctypes.addressof(word), ctypes.addressof(word),
                 ctypes.addressof(word), 4, bufs, one, 64, 2, 0, None, None, None) == L.DV_ERR_ARG, n_lanes
