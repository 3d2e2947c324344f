"""The closed-form TPC-C epochs of tests/adversarial_tpcc.py against the CPU
oracle (O.TpccDB.epoch): commit bytes, o_ids, committed / write counts and
every column of the five tables after every epoch.

A disagreement here means the oracle or the formula is wrong; the ruling is
settled from the reference's text (run_payment_1/3/5 and new_order_5/9,
tpcc_txn.cpp:530-933).  Every formula agrees with the oracle as committed; no
ruling was needed.  Empty TPC-C txns: the oracle accepts them and they commit
(family 5 follows it, as adversarial.ladder(empties=True) does for YCSB).

The second half shows, family by family, that the formula separates the
correct result from the mistake the family exists to catch.  Each mistake is a
small Python model of what k_tpcc_apply / k_tpcc_oid (csrc/dvcc_tpcc.hip)
would compute if it were wrong in that way, over this module's own sort of the
epoch -- never a change to project code.
"""
import numpy as np
import pytest

import _oracle as O
import adversarial_tpcc as AT
from adversarial_tpcc import T_CUST, T_DIST, T_STOCK

OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}


def _hold(case, cc):
    db = O.TpccDB(case.cx.po, AT.LOAD_SEED)
    state = case.cx.init()
    for k, e in enumerate(case.epochs):
        c, oid, committed, wcnt, state = case.expect(cc, k, state)
        c_ref, o_ref, st = db.epoch(OCC_ID[cc], e.keys, e.types, e.tables, e.args, e.txn_begin)
        bad = np.flatnonzero(c_ref != c)
        assert bad.size == 0, f"{cc} epoch {k}: oracle and formula differ at txns {bad[:8]} ({bad.size} in all)"
        assert np.array_equal(o_ref, oid), f"{cc} epoch {k}: o_id differs at {np.flatnonzero(o_ref != oid)[:8]}"
        assert (st.committed, st.aborted, st.write_cnt) == (committed, e.n_txn - committed, wcnt), (cc, k)
        for t in range(5):
            ref = db.table(t)
            for col in range(3):
                d = np.flatnonzero(ref[1 + col] != state[t][col])
                assert d.size == 0, f"{cc} epoch {k}: table {t} col {col} differs at rows {d[:8]}"


@pytest.mark.parametrize("cc", AT.CCS)
@pytest.mark.parametrize("name", list(AT.CASES))
def test_family_against_oracle(name, cc):
    _hold(AT.built(name), cc)


@pytest.mark.parametrize("cc", AT.CCS)
@pytest.mark.parametrize("kind", AT.SWEEPS)
def test_second_sweep_against_oracle(kind, cc):
    _hold(AT.built_sweep(kind), cc)


def test_sweep_geometry_parses():
    S = AT.sweep()
    assert S > 0 and S % AT.A.structural_constants()["kBlock"] == 0


def test_stale_cases_all_occur():
    """family 6's builder asserts (a), (b) and (c); this names them"""
    kinds = {x[3] for x in AT.built("stale").extra["stale"]}
    assert kinds == {"a", "b", "c"}


# ---- the mistakes, as models over the sorted epoch (CALVIN: every txn applied)
def _runs(g):
    """[start, end) of every row's run in the sorted rows g"""
    start = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
    return start, np.r_[start[1:], len(g)]


def _lane_edge_sum(sv, row):
    """W_YTD / D_YTD / C_BALANCE delta of `row` when a run's sum drops what lies
    past the 64-lane edge after the run's first access"""
    at = np.flatnonzero(sv.g == row)
    a, b = int(at[0]), int(at[-1]) + 1
    cut = min(b, (a // 64 + 1) * 64)
    return a, b, int(sv.v[a:cut].astype(np.int64).sum())


STORMS = [n for n in AT.CASES if n.startswith("storm_") and not n.endswith("_rdwh")]


@pytest.mark.parametrize("name", STORMS)
def test_model_lane_edge_is_separated(name):
    """a run sum that drops what lies past a 64-lane edge: wrong on every run
    that crosses an edge.  The three runs are [k, k + m), [k + m, k + 2m) and
    [k + 2m, k + 3m) behind k fillers, so every storm of more than 2 Payments
    has such a run but m = 64 without fillers, whose runs are whole waves"""
    case = AT.built(name)
    cx, e = case.cx, case.epochs[0]
    sv = AT.sorted_view(cx, e)
    before = cx.init()
    _, _, _, _, after = case.expect("CALVIN", 0, before)
    crossed = 0
    for t, r in case.extra["rows"].values():
        a, b, s = _lane_edge_sum(sv, int(cx.base[t]) + r)
        want = abs(AT._f(after[t][0][r]) - AT._f(before[t][0][r]))
        crosses = (b - 1) // 64 != a // 64
        assert (s != want) == crosses, (name, t, a, b)
        crossed += crosses
    m = len(case.extra["h"])
    assert (crossed > 0) == (m > 2 and (m != 64 or case.extra["fillers"] % 64 != 0)), name


@pytest.mark.parametrize("name", ["districts", "districts_alone"])
def test_model_rank_restart_is_separated(name):
    """a rank that restarts at each step of 64 (the count of earlier steps
    dropped): every district whose NewOrders reach a second step gets wrong
    o_ids and a wrong D_NEXT_O_ID"""
    case = AT.built(name)
    cx, e = case.cx, case.epochs[0]
    sv = AT.sorted_view(cx, e)
    before = cx.init()
    _, oid, _, _, after = case.expect("CALVIN", 0, before)
    wrong_oid = np.zeros_like(oid)
    wrong = 0
    for a, b in zip(*_runs(sv.g)):
        if sv.tab[a] != T_DIST:
            continue
        r = int(sv.g[a] - cx.base[T_DIST])
        snap = int(before[T_DIST][1][r])
        last = 0
        for s0 in range(a, b, 64):
            no = np.flatnonzero(sv.op[s0:min(b, s0 + 64)] == AT.OP_NO_DIST)
            wrong_oid[sv.txn[s0 + no]] = snap + 1 + np.arange(len(no))
            last = len(no)
        long_q = int((sv.op[a + 64:b] == AT.OP_NO_DIST).sum()) > 0
        assert (snap + last != int(after[T_DIST][1][r])) == long_q
        wrong += long_q
    assert wrong >= 5 and not np.array_equal(wrong_oid, oid)


def _chain_model(s, qs, rule):
    for q in qs:
        s = rule(s, q)
    return s


@pytest.mark.parametrize("m", [1, 64, 65, 300])
def test_model_stock_rule_is_separated(m):
    """`>=` for `>` (wrong at s == q + 10: item A's last write) and a threshold
    one higher (wrong at s == q + 11: item B's): the pair tells each from the
    rule"""
    case = AT.built(f"chain_{m}")
    cx = case.cx
    before = cx.init()
    _, _, _, _, after = case.expect("CALVIN", 0, before)
    want = [int(after[T_STOCK][0][r]) for r in case.extra["rows"]]
    for rule in (lambda s, q: s - q if s >= q + 10 else s - q + 91,
                 lambda s, q: s - q if s > q + 11 else s - q + 91):
        got = [_chain_model(int(before[T_STOCK][0][r]), qs, rule) for r, qs in zip(case.extra["rows"], case.extra["q"])]
        assert got != want
    assert got[0] == want[0] and got[1] != want[1]  # (the second mistake shows on item B alone)
    assert want == [_chain_model(int(before[T_STOCK][0][r]), qs, AT.stock_rule)
                    for r, qs in zip(case.extra["rows"], case.extra["q"])]


def test_model_stale_start_accepted_is_separated():
    """a stale start that is accepted: the wave of an absent district numbers
    the queue it finds at its old index from its old snapshot and stores the
    grown word into its own row.  Wrong wherever that index holds another
    district's queue with a NewOrder in it -- case (a)"""
    case = AT.built("stale")
    cx = case.cx
    state = cx.init()
    snaps = {}  # district row -> D_NEXT_O_ID at its last recorded head
    hit = 0
    for k, e in enumerate(case.epochs):
        sv = AT.sorted_view(cx, e)
        _, _, _, _, after = case.expect("CALVIN", k, state)
        for kk, d, i0, kind in case.extra["stale"]:
            if kk != k or kind == "c":
                continue
            j = i0
            while j < len(sv.g) and sv.g[j] == sv.g[i0]:
                j += 1
            count = int((sv.op[i0:j] == AT.OP_NO_DIST).sum())
            if count:
                assert kind == "a"
                assert snaps[d] + count != int(after[T_DIST][1][d]), "the accepted stale start is not told apart"
                hit += 1
        for i in np.flatnonzero(sv.head() & (sv.tab == T_DIST)):
            d = int(sv.g[i] - cx.base[T_DIST])
            snaps[d] = int(state[T_DIST][1][d])
        state = after
    assert hit > 0


@pytest.mark.parametrize("kind", AT.SWEEPS)
def test_model_sweep_stops_is_separated(kind):
    """a sweep that stops at 4,096 x kBlock accesses: the additive run that
    straddles the index loses its tail, and the stock queues whose heads lie
    beyond it are never walked"""
    case = AT.built_sweep(kind)
    cx, e = case.cx, case.epochs[0]
    S = case.extra["S"]
    sv = AT.sorted_view(cx, e)
    before = cx.init()
    _, _, _, _, after = case.expect("CALVIN", 0, before)
    wrong = 0
    if kind == "cust":
        r = int(sv.g[S] - cx.base[T_CUST])
        at = np.flatnonzero(sv.g[:S] == sv.g[S])
        got = AT._f(before[T_CUST][1][r]) + float(sv.v[at].astype(np.int64).sum())
        assert got != AT._f(after[T_CUST][1][r])
        wrong += 1
    for i in np.flatnonzero(sv.head() & (sv.tab == T_STOCK)):
        if i >= S:  # (never reached: the row keeps its loaded values)
            r = int(sv.g[i] - cx.base[T_STOCK])
            assert any(int(after[T_STOCK][c][r]) != int(before[T_STOCK][c][r]) for c in range(3))
            wrong += 1
    assert wrong >= 2
