"""Closed-form adversarial TPC-C epochs (a plain module, shared by
test_adversarial_tpcc_cpu.py and test_adversarial_tpcc_gpu.py).

tests/adversarial.py pins the decision kernels with epochs whose commit set is
a formula; this module does the same for TPC-C's execution kernels,
k_tpcc_apply and k_tpcc_oid (csrc/dvcc_tpcc.hip).  Every family builds hand-
made epochs (keys, types, tables, args, txn_begin) and states, per CC
algorithm, which txns are applied -- a rule, never the oracle's or the
engine's output:
  NO_WAIT / WAIT_DIE / OCC   the first writer of a row in sequence order
                             commits, later ones abort (every family's txns
                             conflict on written rows only)
  CALVIN                     all commit.
The table state then follows row by row from the applied set (`_aggregate`):
  W_YTD, D_YTD              += sum of h            (run_payment_1/3)
  C_BALANCE                 -= sum of h, C_YTD_PAYMENT += sum of h,
  C_PAYMENT_CNT             += count, from the integer-1 bit pattern the loader
                            leaves (a denormal double; + 1.0 gives 1.0 exactly,
                            as oracle/tpcc.c restates run_payment_5)
  D_NEXT_O_ID               += applied NewOrders of the district; the j-th of
                            them in sequence order takes D_NEXT_O_ID + j
  S_QUANTITY                s > q + 10 ? s - q : s - q + 91 in sequence order,
                            S_YTD += sum of q, S_ORDER_CNT += count (new_order_9)
and every family adds the closed form of its headline values (sum of h as
m (m + 1) / 2 ...) as assertions of its own (`closed`).  Initial values are
read from the loaded tables, never written down here.

Op words are well formed, as tpcc_gen.cpp emits them: each op on its own table
with type WR (the kernel ignores an op word that names another table; the
oracle does not).  Operands are distinct powers of two where a family is small
(the final value then names the applied txns), h_j = j + 1 elsewhere.

Row order: the engine's row_base grows with the table id (dv_tpcc_load creates
the tables in id order, each at total_rows) and every table is loaded in key
order, so the sorted pairs are ordered by (table id, key); `sorted_view` is a
stable sort by that, and the builders assert the positions they are after.
"""
import functools
import re
from dataclasses import dataclass, field

import numpy as np

import _oracle as O
import adversarial as A
from dvcc import tpcc as T

CCS = A.CCS
PARAMS = dict(num_wh=2, cust_per_dist=1000, max_items=2000)
LOAD_SEED = 5
T_WH, T_DIST, T_CUST, T_ITEM, T_STOCK, T_CLAST = range(6)
OP_NONE, OP_PAY_WH, OP_PAY_DIST, OP_PAY_CUST, OP_NO_DIST, OP_NO_STOCK = range(6)
RD, WR = 0, 1
OP_MASK = (1 << 56) - 1


def sweep():
    """accesses one sweep of k_tpcc_apply covers: grid_for's 4,096 blocks of
    kBlock threads (csrc/dvcc_tpcc.hip)"""
    cap = int(re.search(r"g > (\d+) \? \1 : g", A._src("dvcc_tpcc.hip")).group(1))
    return cap * A.structural_constants()["kBlock"]


class Ctx:
    """the loaded tables of one parameter set: keys (sorted), initial columns
    and each table's first global row"""

    def __init__(self, **kw):
        self.kw = dict(PARAMS, **kw)
        self.po = O.tpcc_params(**self.kw)
        db = O.TpccDB(self.po, LOAD_SEED)
        tabs = [db.table(t) for t in range(5)]
        self.keys = [t[0] for t in tabs]
        self._init = [[c for c in t[1:]] for t in tabs]
        for k in self.keys:
            assert (np.diff(k.astype(np.int64)) > 0).all(), "a table is not loaded in key order"
        self.base = np.r_[0, np.cumsum([len(k) for k in self.keys])].astype(np.int64)

    def pp(self):
        return T.tpcc_params(**self.kw)

    def init(self):
        return copy_state(self._init)

    def row(self, t, key):
        key = np.asarray(key, np.uint64)
        r = np.searchsorted(self.keys[t], key)
        assert (self.keys[t][np.minimum(r, len(self.keys[t]) - 1)] == key).all(), f"no such key in table {t}"
        return r

    # keys (tpcc_helper.cpp:19-43)
    def k_dist(self, d, w):
        return w * 10 + d

    def k_cust(self, c, d, w):
        return self.k_dist(d, w) * self.kw["cust_per_dist"] + c

    def k_stock(self, i, w):
        return w * self.kw["max_items"] + i


@functools.lru_cache(maxsize=None)
def ctx(wh_update=1):
    return Ctx(wh_update=wh_update)


def copy_state(s):
    return [[c.copy() for c in t] for t in s]


# ---- accesses and epochs
def a_wh(w, h, upd=True):
    return (T_WH, w, WR, OP_PAY_WH, h) if upd else (T_WH, w, RD, OP_NONE, h)


def a_wh_rd(w):
    return (T_WH, w, RD, OP_NONE, 0)


def a_pdist(kd, h):
    return (T_DIST, kd, WR, OP_PAY_DIST, h)


def a_pcust(kc, h):
    return (T_CUST, kc, WR, OP_PAY_CUST, h)


def a_plast(knp, h):
    return (T_CLAST, knp, WR, OP_PAY_CUST, h)


def a_nodist(kd):
    return (T_DIST, kd, WR, OP_NO_DIST, 0)


def a_stock(ks, q):
    return (T_STOCK, ks, WR, OP_NO_STOCK, q)


class _EB:
    def __init__(self):
        self.acc, self.lens = [], []

    def txn(self, *accs):
        self.acc += accs
        self.lens.append(len(accs))
        return len(self.lens) - 1

    def epoch(self):
        a = np.array(self.acc, dtype=np.uint64).reshape(-1, 5)
        return _epoch(self.lens, a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4])


def _epoch(lens, tables, keys, types, ops, vals):
    tb = np.zeros(len(lens) + 1, np.uint32)
    tb[1:] = np.cumsum(lens)
    vals = np.asarray(vals, np.uint64)
    assert int(tb[-1]) == len(keys) and (len(vals) == 0 or int(vals.max()) < 1 << 40)
    args = (np.asarray(ops, np.uint64) << np.uint64(56)) | vals
    return T.TpccEpoch(np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(types, dtype=np.uint8), tb,
                       np.ascontiguousarray(tables, dtype=np.uint8), np.ascontiguousarray(args, dtype=np.uint64))


def _amounts(m):
    """distinct powers of two where the family is small, h_j = j + 1 elsewhere"""
    j = np.arange(m, dtype=np.uint64)
    return (np.uint64(1) << j) if m <= 40 else j + np.uint64(1)


@dataclass
class SortedView:
    g: np.ndarray      # global row of every sorted access
    tab: np.ndarray    # its table (last names resolved to CUSTOMER)
    txn: np.ndarray
    op: np.ndarray
    v: np.ndarray
    order: np.ndarray  # sorted position -> access index

    def head(self):
        return np.r_[True, self.g[1:] != self.g[:-1]]


def resolved(cx, e, resolve=None):
    """(table, row in table) of every access; a last-name key through
    `resolve` (custNPKey -> custKey)"""
    tab, key = e.tables.copy(), e.keys.copy()
    last = tab == T_CLAST
    if last.any():
        key[last] = [resolve[int(k)] for k in key[last]]
        tab[last] = T_CUST
    row = np.zeros(len(key), np.int64)
    for t in range(5):
        m = tab == t
        if m.any():
            row[m] = cx.row(t, key[m])
    return tab, row


def sorted_view(cx, e, resolve=None):
    """the epoch's accesses as the engine sorts them: stable by table id, then
    row index (sequence order within a row)"""
    tab, row = resolved(cx, e, resolve)
    g = cx.base[tab] + row
    order = np.argsort(g, kind="stable")
    return SortedView(g[order], tab[order], e.acc_txn()[order], (e.args >> np.uint64(56))[order],
                      (e.args & np.uint64(OP_MASK))[order], order)


def stock_rule(s, q):
    return s - q if s > q + 10 else s - q + 91


def _aggregate(cx, e, applied, before, resolve=None):
    """the state after the applied txns, row by row (module docstring), and
    every txn's o_id"""
    after = copy_state(before)
    tab, row = resolved(cx, e, resolve)
    txn = e.acc_txn()
    op = e.args >> np.uint64(56)
    v = (e.args & np.uint64(OP_MASK)).astype(np.int64)
    assert len(v) == 0 or int(v.max()) < 1 << 40
    on = applied[txn].astype(bool)
    assert ((op == OP_NONE) | (e.types == WR)).all()
    for o, t in ((OP_PAY_WH, T_WH), (OP_PAY_DIST, T_DIST), (OP_PAY_CUST, T_CUST), (OP_NO_DIST, T_DIST),
                 (OP_NO_STOCK, T_STOCK)):
        assert (tab[op == o] == t).all(), "an op word on another table"
    for o, t in ((OP_PAY_WH, T_WH), (OP_PAY_DIST, T_DIST)):
        m = on & (op == o)
        np.add.at(after[t][0].view(np.float64), row[m], v[m].astype(np.float64))
    m = on & (op == OP_PAY_CUST)
    np.add.at(after[T_CUST][0].view(np.float64), row[m], -v[m].astype(np.float64))
    np.add.at(after[T_CUST][1].view(np.float64), row[m], v[m].astype(np.float64))
    np.add.at(after[T_CUST][2].view(np.float64), row[m], 1.0)
    oid = np.zeros(e.n_txn, np.uint64)
    nxt = after[T_DIST][1]
    for a in np.flatnonzero(on & (op == OP_NO_DIST)):  # (sequence order)
        nxt[row[a]] += np.uint64(1)
        oid[txn[a]] = nxt[row[a]]
    m = np.flatnonzero(on & (op == OP_NO_STOCK))
    if m.size:
        r = row[m]
        o = np.argsort(r, kind="stable")
        r, q = r[o], v[m][o]
        start = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
        rank = np.arange(len(r)) - np.repeat(start, np.diff(np.r_[start, len(r)]))
        s0, s1, s2 = (after[T_STOCK][c].view(np.int64) for c in range(3))
        by_rank = np.argsort(rank, kind="stable")
        cut = np.r_[0, np.cumsum(np.bincount(rank))]
        for lv in range(len(cut) - 1):  # the lv-th applied access of every row, all rows at once
            sel = by_rank[cut[lv]:cut[lv + 1]]
            rr, qq = r[sel], q[sel]
            s = s0[rr]
            s0[rr] = np.where(s > qq + 10, s - qq, s - qq + 91)
            s1[rr] += qq
            s2[rr] += 1
    return oid, after


def write_count(e, commit):
    per_txn = np.bincount(e.acc_txn(), weights=(e.types == WR), minlength=e.n_txn).astype(np.int64)
    return int((per_txn * commit.astype(np.int64)).sum())


@dataclass
class TCase:
    """epochs: run in order on one database.  applied(cc, k): the commit bytes
    of epoch k (uint8).  closed(cc, k, before, after, oid): the family's closed
    forms, asserted on the aggregated expectation."""
    cx: Ctx
    epochs: list
    applied: object
    closed: object = None
    resolve: dict = None
    extra: dict = field(default_factory=dict)

    def expected_commit(self, cc, k=0):
        c = self.applied(cc, k)
        assert c.dtype == np.uint8 and len(c) == self.epochs[k].n_txn
        return c

    def expect(self, cc, k, before):
        """(commit, o_id, committed, write_cnt, tables after) of epoch k run
        on the state `before`"""
        e = self.epochs[k]
        c = self.expected_commit(cc, k)
        oid, after = _aggregate(self.cx, e, c, before, self.resolve)
        if self.closed is not None:
            self.closed(cc, k, before, after, oid)
        return c, oid, int(c.sum()), write_count(e, c), after


def _f(bits):
    return float(np.uint64(bits).view(np.float64))


def _first_only(n, firsts):
    c = np.zeros(n, np.uint8)
    c[list(firsts)] = 1
    return c


# ---- family 1: Payment storm(m, fillers, wh_update).  `fillers` single-access
# txns on warehouse 1's row (the lowest row of all), then m Payments on
# warehouse 2, one district and one customer: in the sorted pairs three runs of
# m accesses, the first starting at index `fillers`.
# CALVIN: W_YTD, D_YTD += sum h; C_BALANCE -= sum h; C_YTD_PAYMENT += sum h;
# C_PAYMENT_CNT = m.  Others: the first Payment's amounts alone (and the first
# filler's; with wh_update = 0 the warehouse accesses are reads: every filler
# commits, W_YTD stays).
def payment_storm(m, fillers=0, wh_update=1):
    cx = ctx(wh_update)
    w, d, c = 2, 3, 17
    h = _amounts(m)
    fh = np.arange(fillers, dtype=np.uint64) + np.uint64(1 << 20)
    b = _EB()
    for i in range(fillers):
        b.txn(a_wh(1, int(fh[i]), wh_update))
    for j in range(m):
        b.txn(a_wh(w, int(h[j]), wh_update), a_pdist(cx.k_dist(d, w), int(h[j])), a_pcust(cx.k_cust(c, d, w), int(h[j])))
    e = b.epoch()
    rw, rw1 = int(cx.row(T_WH, w)), int(cx.row(T_WH, 1))
    rd, rc = int(cx.row(T_DIST, cx.k_dist(d, w))), int(cx.row(T_CUST, cx.k_cust(c, d, w)))

    def applied(cc, k):
        if cc == "CALVIN":
            return np.ones(e.n_txn, np.uint8)
        c = _first_only(e.n_txn, [fillers])  # the first Payment
        if wh_update:
            c[:min(fillers, 1)] = 1  # the fillers write one row: the first of them
        else:
            c[:fillers] = 1  # ... or read it: all of them
        return c

    def closed(cc, k, before, after, oid):
        all_ = cc == "CALVIN"
        sh = int(h.sum()) if all_ else int(h[0])
        assert not all_ or m > 40 or sh == (1 << m) - 1
        assert not all_ or m <= 40 or sh == m * (m + 1) // 2
        cnt = m if all_ else 1
        sf = 0 if not (fillers and wh_update) else (int(fh.sum()) if all_ else int(fh[0]))
        assert _f(after[T_WH][0][rw]) == _f(before[T_WH][0][rw]) + (sh if wh_update else 0)
        assert _f(after[T_WH][0][rw1]) == _f(before[T_WH][0][rw1]) + sf
        assert _f(after[T_DIST][0][rd]) == _f(before[T_DIST][0][rd]) + sh
        assert _f(after[T_CUST][0][rc]) == _f(before[T_CUST][0][rc]) - sh
        assert _f(after[T_CUST][1][rc]) == _f(before[T_CUST][1][rc]) + sh
        assert _f(after[T_CUST][2][rc]) == _f(before[T_CUST][2][rc]) + cnt
        if int(before[T_CUST][2][rc]) == 1:  # the loader's integer 1: the count itself, as a double
            assert _f(after[T_CUST][2][rc]) == float(cnt)
        assert not oid.any()

    return TCase(cx, [e], applied, closed, extra=dict(h=h, fillers=fillers, rows=dict(wh=(T_WH, rw), dist=(T_DIST, rd), cust=(T_CUST, rc))))


# ---- family 2: by id and by last name(m).  m Payments [DISTRICT, customer],
# the customer alternately as CUSTOMER/custKey and CUST_LAST/custNPKey, both the
# same row.  The last-name key comes from a generated all-Payment epoch; the
# customer it resolves to from that one access run alone on a scratch oracle
# database (the row whose C_YTD_PAYMENT changed).  Same rules as family 1.
@functools.lru_cache(maxsize=None)
def last_name_pair():
    cx = ctx()
    keys, _, tables, *_ = O.tpcc_gen(O.tpcc_params(**dict(cx.kw, perc_payment=1.0)), 64, 77)
    at = np.flatnonzero(tables == T_CLAST)
    assert at.size, "no Payment by last name in the generated epoch"
    knp = int(keys[at[0]])
    one = _epoch([1], [T_CLAST], [knp], [WR], [OP_PAY_CUST], [1])
    db = O.TpccDB(cx.po, LOAD_SEED)
    db.epoch(O.CALVIN, one.keys, one.types, one.tables, one.args, one.txn_begin)
    rows = np.flatnonzero(db.table(T_CUST)[2] != cx._init[T_CUST][1])
    assert rows.size == 1
    return knp, int(cx.keys[T_CUST][rows[0]])


def by_id_and_name(m):
    cx = ctx()
    knp, kc = last_name_pair()
    kd = (kc - 1) // cx.kw["cust_per_dist"]
    h = _amounts(m)
    b = _EB()
    for j in range(m):
        b.txn(a_pdist(kd, int(h[j])), a_pcust(kc, int(h[j])) if j % 2 == 0 else a_plast(knp, int(h[j])))
    e = b.epoch()
    rc, rd = int(cx.row(T_CUST, kc)), int(cx.row(T_DIST, kd))

    def applied(cc, k):
        return np.ones(m, np.uint8) if cc == "CALVIN" else _first_only(m, [0])

    def closed(cc, k, before, after, oid):
        sh, cnt = (int(h.sum()), m) if cc == "CALVIN" else (int(h[0]), 1)
        assert _f(after[T_DIST][0][rd]) == _f(before[T_DIST][0][rd]) + sh
        assert _f(after[T_CUST][0][rc]) == _f(before[T_CUST][0][rc]) - sh
        assert _f(after[T_CUST][1][rc]) == _f(before[T_CUST][1][rc]) + sh
        assert _f(after[T_CUST][2][rc]) == _f(before[T_CUST][2][rc]) + cnt

    return TCase(cx, [e], applied, closed, resolve={knp: kc})


# ---- district epochs (families 3 and 6).  queues: [(district key, events)],
# events a string of 'N' (NewOrder) and 'P' (Payment) in the district's own
# sequence order; the txns of all districts are dealt round-robin, so every
# queue is interleaved with every other in sequence order.
#   NewOrder  [WAREHOUSE read]? DISTRICT/NO_DIST, STOCK/NO_STOCK on an item of
#             its own
#   Payment   DISTRICT/PAY_DIST h, CUSTOMER/PAY_CUST h on a customer of its own
# (alone: the district access only).  The first `wh_reads` NewOrders read their
# warehouse row (reads never conflict: no txn writes a warehouse here).
# Only district rows are shared, so under NO_WAIT / WAIT_DIE / OCC the first txn
# of each district commits and the rest abort.
def _spread(q, p, p_first):
    n = q + p
    ev = ["P" if (i * p) // n != ((i + 1) * p) // n else "N" for i in range(n)]
    return "".join(ev[::-1] if p_first else ev)


def _district_epoch(cx, queues, alone=False, wh_reads=0, salt=0):
    b = _EB()
    firsts, info = [], {}
    cur = [0] * len(queues)
    item = cust = 0
    pay_no = {kd: 0 for kd, _ in queues}
    live = True
    while live:
        live = False
        for qi, (kd, ev) in enumerate(queues):
            if cur[qi] >= len(ev):
                continue
            live = True
            w, d = (kd - 1) // 10, (kd - 1) % 10 + 1
            acc = []
            if ev[cur[qi]] == "N":
                if wh_reads:
                    acc.append(a_wh_rd(w))
                    wh_reads -= 1
                acc.append(a_nodist(kd))
                if not alone:
                    item += 1
                    acc.append(a_stock(cx.k_stock(item, w), 1 + (item + salt) % 10))
            else:
                p_cnt = ev.count("P")
                hj = int(_amounts(p_cnt)[pay_no[kd]]) if p_cnt <= 40 else pay_no[kd] + 1
                pay_no[kd] += 1
                acc.append(a_pdist(kd, hj))
                if not alone:
                    cust += 1
                    acc.append(a_pcust(cx.k_cust(cust, d, w), hj))
            t = b.txn(*acc)
            if cur[qi] == 0:
                firsts.append(t)
            info.setdefault(kd, []).append((t, ev[cur[qi]]))
            cur[qi] += 1
    assert item <= cx.kw["max_items"] and cust <= cx.kw["cust_per_dist"]
    return b.epoch(), firsts, info


def _district_closed(cx, infos):
    def closed(cc, k, before, after, oid):
        for kd, evs in infos[k].items():
            r = int(cx.row(T_DIST, kd))
            ap = evs if cc == "CALVIN" else evs[:1]
            nos = [t for t, x in ap if x == "N"]
            first = int(before[T_DIST][1][r])
            # the j-th NewOrder of the district takes D_NEXT_O_ID + j; the row ends at + q_d
            assert [int(oid[t]) for t in nos] == list(range(first + 1, first + 1 + len(nos)))
            assert int(after[T_DIST][1][r]) == first + len(nos)
            assert all(int(oid[t]) == 0 for t, _ in evs if t not in nos)  # (Payments and aborted txns: none)
    return closed


# ---- family 3: district queues.  Seven districts of warehouse 1, q_d
# NewOrders and p_d Payments in district d's queue (the Payments sit in the
# queue, take no o_id): the queues are 2, 64, 128, 128, 192, 132 and 256 long,
# so k_tpcc_oid's steps of 64 end inside a step, exactly on a step edge (one,
# two, three and four steps) and past one.  alone: district accesses only, so
# the last queue -- four whole steps -- ends at n and the next step starts there.
Q_NO = (1, 63, 64, 65, 128, 129, 200)
Q_PAY = (1, 1, 64, 63, 64, 3, 56)


def district_queues(alone=False):
    cx = ctx()
    queues = [(cx.k_dist(d + 1, 1), _spread(q, p, d % 2 == 0)) for d, (q, p) in enumerate(zip(Q_NO, Q_PAY))]
    e, firsts, info = _district_epoch(cx, queues, alone=alone)
    sv = sorted_view(cx, e)
    if alone:
        assert (sv.tab == T_DIST).all() and (sv.g[-(Q_NO[-1] + Q_PAY[-1]):] == sv.g[-1]).all(), "the last queue is to end at n"
    assert {ev[0] for _, ev in queues} == {"N", "P"}, "queues are to start with either kind"

    def applied(cc, k):
        return np.ones(e.n_txn, np.uint8) if cc == "CALVIN" else _first_only(e.n_txn, firsts)

    return TCase(cx, [e], applied, _district_closed(cx, [info]), extra=dict(info=info))


# ---- family 4: stock chain(m).  Two items adjacent in row order, m single-
# access NewOrder stock writes on each, alternating in sequence order: in the
# sorted pairs item A's queue [0, m) ends where item B's [m, 2m) begins.  The
# items are the first adjacent pair whose loaded S_QUANTITY lets A's first
# write hit s == q + 10 (the + 91 branch) and B's hit s == q + 11 (the other);
# each chain's last write meets the same edge again (_chain).
# CALVIN: S_QUANTITY by the rule in order, S_YTD += sum q, S_ORDER_CNT += m.
# Others: the first write of each item alone.
def _steer(s, steps, lo, hi):
    """`steps` quantities (1..10 each) that take S_QUANTITY from s into [lo, hi]"""
    levels, level = [], {s: None}
    for _ in range(steps):
        nxt = {}
        for x in level:
            for q in range(1, 11):
                nxt.setdefault(stock_rule(x, q), (x, q))
        levels.append(nxt)
        level = nxt
    goal = [y for y in sorted(level) if lo <= y <= hi]
    assert goal, "no way to the edge"
    y, qs = goal[0], []
    for nxt in reversed(levels):
        y, q = nxt[y]
        qs.append(q)
    return qs[::-1]


def _chain(s, m, edge):
    """m quantities whose first and last both meet s == q + edge; in between
    1..10 in a cycle, back to an edge whenever s allows, and the last steps
    steered to where the final one can meet its edge.  (A wrong branch taken
    mid-chain heals at the next wrap -- both values then differ by 91 until the
    smaller one takes the + 91 branch -- so only the LAST access of a chain
    shows in S_QUANTITY; that is why the edges sit there.)"""
    assert m == 1 or m >= 3
    mid = max(0, m - 2)
    free = mid - min(mid, 24)
    qs, seen = [], set()
    for j in range(m):
        if j == 0 or j == m - 1:
            q = s - edge
        elif j - 1 < free:
            q = s - 11 if 12 <= s <= 21 and j % 2 == 0 else (s - 10 if 11 <= s <= 20 else 1 + (7 * j) % 10)
        else:
            if j - 1 == free:
                plan = _steer(s, mid - free, edge + 1, edge + 10)
            q = plan[j - 1 - free]
        assert 1 <= q <= 10
        seen.add("gt" if s > q + 10 else "le")
        if s == q + 10:
            seen.add("e10")
        if s == q + 11:
            seen.add("e11")
        qs.append(q)
        s = stock_rule(s, q)
    return qs, s, seen


def stock_chain(m):
    cx = ctx()
    k, s0 = cx.keys[T_STOCK].astype(np.int64), cx._init[T_STOCK][0].astype(np.int64)
    ok = (k[1:] == k[:-1] + 1) & (s0[:-1] >= 11) & (s0[:-1] <= 20) & (s0[1:] >= 12) & (s0[1:] <= 21)
    assert ok.any(), "no adjacent pair of items with S_QUANTITY at the two edges"
    ra = int(np.flatnonzero(ok)[0])
    qa, sa, fa = _chain(int(s0[ra]), m, 10)
    qb, sb, fb = _chain(int(s0[ra + 1]), m, 11)
    assert fa | fb == {"gt", "le", "e10", "e11"}, "both branches and both edges are to occur"
    b = _EB()
    for j in range(m):
        b.txn(a_stock(int(k[ra]), qa[j]))
        b.txn(a_stock(int(k[ra + 1]), qb[j]))
    e = b.epoch()
    sv = sorted_view(cx, e)
    assert (sv.g[:m] == sv.g[0]).all() and (sv.g[m:] == sv.g[0] + 1).all()

    def applied(cc, _k):
        return np.ones(2 * m, np.uint8) if cc == "CALVIN" else _first_only(2 * m, [0, 1])

    def closed(cc, _k, before, after, oid):
        for r, qs, s_end in ((ra, qa, sa), (ra + 1, qb, sb)):
            if [int(before[T_STOCK][c][r]) for c in range(3)] != [int(cx._init[T_STOCK][c][r]) for c in range(3)]:
                continue  # (the quantities were chosen for the loaded values)
            n = m if cc == "CALVIN" else 1
            want = s_end if cc == "CALVIN" else stock_rule(int(s0[r]), qs[0])
            assert [int(after[T_STOCK][c][r]) for c in range(3)] == [want, sum(qs[:n]), n]

    return TCase(cx, [e], applied, closed, extra=dict(rows=(ra, ra + 1), q=(qa, qb)))


# ---- family 5: sparse(n_txn).  Three txns with accesses (the first, the middle
# and the last), the rest empty, n_txn / 16 > n_acc: k_tpcc_apply's grid is
# sized by the commit bytes, not the accesses.  The three touch disjoint rows
# and empty txns commit (as adversarial.ladder(empties=True) has it for YCSB):
# every commit byte is 1 under every algorithm.
def sparse(n_txn):
    cx = ctx()
    if n_txn < 1024:
        carriers = [[a_nodist(cx.k_dist(1, 1))], [a_pdist(cx.k_dist(1, 2), 1 << 5)], [a_stock(cx.k_stock(7, 1), 3)]]
    else:
        h = 1 << 7
        no = [a_wh_rd(2), (T_CUST, cx.k_cust(9, 4, 2), RD, OP_NONE, 0), a_nodist(cx.k_dist(4, 2))]
        for i in range(5):
            no += [(T_ITEM, 11 + i, RD, OP_NONE, 0), a_stock(cx.k_stock(11 + i, 2), 1 + i)]
        carriers = [[a_wh(1, h), a_pdist(cx.k_dist(1, 1), h), a_pcust(cx.k_cust(5, 1, 1), h)], no,
                    [a_stock(cx.k_stock(7, 1), 3)]]
    at = {0: 0, n_txn // 2: 1, n_txn - 1: 2}
    lens = np.zeros(n_txn, np.int64)
    acc = []
    for t in sorted(at):
        lens[t] = len(carriers[at[t]])
        acc += carriers[at[t]]
    a = np.array(acc, dtype=np.uint64)
    e = _epoch(lens, a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4])
    assert (n_txn + 15) // 16 > e.n_acc and n_txn // 16 > e.n_acc

    def applied(cc, k):
        return np.ones(n_txn, np.uint8)

    def closed(cc, k, before, after, oid):
        changed = sum(int((np.stack(after[t]) != np.stack(before[t])).any(0).sum()) for t in range(5))
        assert changed == (3 if n_txn < 1024 else 3 + 1 + 5 + 1)
        assert int((oid != 0).sum()) == 1

    return TCase(cx, [e], applied, closed)


# ---- family 6: stale starts.  Nine epochs; epoch k touches district set
# S_(k mod 3), three disjoint sets of six districts.  k_tpcc_apply records where
# each present district's queue starts; a district absent from the next epoch
# leaves its old index behind, and the three shapes make that index hold
#   (a) another district's row     (b) a non-district row
#   (c) nothing (the epoch is shorter than the index)
#   shape 0  no warehouse reads, queues of 40+   districts at [0, 240+)
#   shape 1  100 warehouse reads, queues of 20+  districts at [100, 220+)
#   shape 2  queues of 2                         24 accesses in all
# An untouched district keeps its D_NEXT_O_ID; touched ones continue their own
# count across epochs (the queues grow by one NewOrder per cycle).
def stale_starts(n_epochs=9):
    cx = ctx()
    dk = cx.keys[T_DIST]
    sets = [[int(x) for x in dk[6 * s:6 * s + 6]] for s in range(3)]
    epochs, firsts, infos = [], [], []
    for k in range(n_epochs):
        cyc = k // 3
        q, p, reads = ((30 + cyc, 10, 0), (15 + cyc, 5, 100), (1, 1, 0))[k % 3]
        e, f, info = _district_epoch(cx, [(kd, _spread(q, p, i % 2 == 1)) for i, kd in enumerate(sets[k % 3])],
                                     wh_reads=reads, salt=k)
        epochs.append(e)
        firsts.append(f)
        infos.append(info)
    # the recorded starts, from this module's own sort: what the index a district
    # recorded in epoch k - 1 holds in epoch k, the next one (it is absent there)
    d0, d1 = int(cx.base[T_DIST]), int(cx.base[T_DIST + 1])
    seen, stale, rec = set(), [], {}
    for k, e in enumerate(epochs):
        sv = sorted_view(cx, e)
        present = set()
        for i in np.flatnonzero(sv.head() & (sv.tab == T_DIST)):
            present.add(int(sv.g[i]))
        for row, (at, i0) in rec.items():
            if at != k - 1 or row in present:
                continue
            kind = "c" if i0 >= len(sv.g) else ("a" if d0 <= sv.g[i0] < d1 else "b")
            seen.add(kind)
            stale.append((k, row - d0, i0, kind))
        for i in np.flatnonzero(sv.head() & (sv.tab == T_DIST)):
            rec[int(sv.g[i])] = (k, int(i))
    assert seen == {"a", "b", "c"}, f"stale starts reach {sorted(seen)} only"

    def applied(cc, k):
        return np.ones(epochs[k].n_txn, np.uint8) if cc == "CALVIN" else _first_only(epochs[k].n_txn, firsts[k])

    inner = _district_closed(cx, infos)

    def closed(cc, k, before, after, oid):
        inner(cc, k, before, after, oid)
        touched = cx.row(T_DIST, np.array(sets[k % 3], np.uint64))
        rest = np.setdiff1d(np.arange(len(dk)), touched)
        assert all((after[T_DIST][c][rest] == before[T_DIST][c][rest]).all() for c in range(3))

    return TCase(cx, epochs, applied, closed, extra=dict(stale=stale, sets=sets, infos=infos))


# ---- family 7: second sweep(kind).  8,400 txns of 125 writes each on the
# same 125 rows -- 1,050,000 accesses, every row's run 8,400 long -- so the
# 125th row's run straddles index 4,096 x kBlock = 1,048,576, where
# k_tpcc_apply's grid-stride loop starts its second trip.
#   kind "cust"   125 customers of one district (PAY_CUST, h = txn + 1 + j): the
#                 additive run of the 125th straddles the index
#   kind "stock"  125 items of warehouse 1 (NO_STOCK, q = 1 + (txn + j) % 10):
#                 the 125th item's queue straddles it
# (one sorted array cannot put a customer run and a stock queue across the same
# index, hence two epochs), and a few small txns follow on rows of their own:
# a Payment on warehouse 2 and two stock writes whose queue heads lie beyond the
# index.  CALVIN: all commit.  Others: the first of the 8,400 and the small
# txns commit.
SWEEP_T, SWEEP_R = 8400, 125


def second_sweep(kind):
    cx = ctx()
    S = sweep()
    Tn, R = SWEEP_T, SWEEP_R
    assert Tn * R > S > Tn * (R - 1) + 8
    t = np.arange(Tn, dtype=np.int64)[:, None]
    j = np.arange(R, dtype=np.int64)[None, :]
    if kind == "cust":
        keys = np.broadcast_to(cx.k_cust(1 + j, 1, 1), (Tn, R))
        tab, op, val = T_CUST, OP_PAY_CUST, t + 1 + j
    else:
        keys = np.broadcast_to(cx.k_stock(1 + j, 1), (Tn, R))
        tab, op, val = T_STOCK, OP_NO_STOCK, 1 + (t + j) % 10
    h = 1 << 9
    small = [[a_wh(2, h), a_pdist(cx.k_dist(1, 2), h), a_pcust(cx.k_cust(5, 1, 2), h)],
             [a_stock(cx.k_stock(R + 1, 1), 5)], [a_stock(cx.k_stock(R + 2, 1), 6)]]
    sa = np.array([a for s in small for a in s], dtype=np.int64)
    n_big = Tn * R
    e = _epoch(np.r_[np.full(Tn, R), [len(s) for s in small]],
               np.r_[np.full(n_big, tab), sa[:, 0]], np.r_[keys.ravel(), sa[:, 1]],
               np.r_[np.full(n_big, WR), sa[:, 2]], np.r_[np.full(n_big, op), sa[:, 3]],
               np.r_[val.ravel(), sa[:, 4]])
    sv = sorted_view(cx, e)
    assert len(sv.g) > S and sv.g[S - 1] == sv.g[S] and sv.tab[S] == tab, f"no {kind} run straddles {S}"
    heads = np.flatnonzero(sv.head() & (sv.tab == T_STOCK))
    assert (heads > S).any(), f"no stock queue head beyond {S}"
    n_small = len(small)

    def applied(cc, k):
        if cc == "CALVIN":
            return np.ones(e.n_txn, np.uint8)
        return _first_only(e.n_txn, [0] + list(range(Tn, Tn + n_small)))

    rows = cx.row(tab, np.asarray(keys[0], np.uint64))

    def closed(cc, k, before, after, oid):
        n = Tn if cc == "CALVIN" else 1
        for jj in (0, R - 1):
            r = int(rows[jj])
            if kind == "cust":
                sh = n * (n + 1) // 2 + n * jj  # sum over txns of (txn + 1 + j)
                assert _f(after[tab][0][r]) == _f(before[tab][0][r]) - sh
                assert _f(after[tab][1][r]) == _f(before[tab][1][r]) + sh
                assert _f(after[tab][2][r]) == _f(before[tab][2][r]) + n
            else:
                qs = [1 + (tt + jj) % 10 for tt in range(n)]
                s = int(before[tab][0][r])
                for q in qs:
                    s = stock_rule(s, q)
                assert [int(after[tab][c][r]) for c in range(3)] == [s, int(before[tab][1][r]) + sum(qs),
                                                                     int(before[tab][2][r]) + n]

    return TCase(cx, [e], applied, closed, extra=dict(S=S, tab=tab))


def engine_max_txn(case):
    """TpccEngine sizes max_acc as 33 accesses a txn: the max_txn that holds
    the case's largest epoch"""
    return max(max(e.n_txn for e in case.epochs), max(-(-e.n_acc // 33) for e in case.epochs), 1)


# ---- every case of both test files, by name
def cases():
    cs = {}
    for m in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025):
        cs[f"storm_{m}"] = functools.partial(payment_storm, m)
    for k in (1, 37):
        for m in (63, 64, 129):
            cs[f"storm_{m}_fill{k}"] = functools.partial(payment_storm, m, fillers=k)
    for m in (2, 65, 257):
        cs[f"storm_{m}_rdwh"] = functools.partial(payment_storm, m, fillers=37 if m == 65 else 0, wh_update=0)
    for m in (2, 130):
        cs[f"name_{m}"] = functools.partial(by_id_and_name, m)
    cs["districts"] = district_queues
    cs["districts_alone"] = functools.partial(district_queues, alone=True)
    for m in (1, 64, 65, 300):
        cs[f"chain_{m}"] = functools.partial(stock_chain, m)
    for n in (4099, 65):
        cs[f"sparse_{n}"] = functools.partial(sparse, n)
    cs["stale"] = stale_starts
    return cs


CASES = cases()
SWEEPS = ("cust", "stock")  # family 7, the only large one: built once, by the tests that run it
# the families that also run partitioned at world 2 (test_adversarial_tpcc_part_gpu.py says why not name_*)
PART_CASES = [n for n in CASES if not n.startswith("name_")]


@functools.lru_cache(maxsize=None)
def built(name):
    return CASES[name]()


@functools.lru_cache(maxsize=2)
def built_sweep(kind):
    return second_sweep(kind)


# ---- family 8: ragged ladder, partitioned(world, slots, own).  The TPC-C
# counterpart of adversarial.ragged_ladder for dv_tpcc_epoch_run_part's list
# protocol: one warehouse per partition (Ctx(num_wh=world), warehouse w on
# partition (w - 1) % world).  `slots` lists the epoch's sequence slots: EMPTY,
# ONE (a single private access) or a pad count p (a ladder txn: the k-th writes
# link rows L_k and L_k+1, then p private accesses; 2 + p <= 33, the longest
# NewOrder).  All accesses are writes with an operation word:
#   link L_k   CUSTOMER (k // m + 1) of district LINK_DIST in link warehouse
#              k % m, OP_PAY_CUST: consecutive links sit on different
#              partitions, so an odd ladder txn loses on L_k's partition while
#              its other records live elsewhere
#   private    used once in the epoch: a CUSTOMER payment (districts 1..9) or,
#              every fifth of a warehouse, a STOCK write; the i-th private
#              access goes to warehouse
#                spread     i % world + 1
#                part0      1
#                skip_last  i % (world - 1) + 1
#              (adversarial.OWNERSHIPS for the private accesses).  Under
#              skip_last at world >= 3 links and districts keep off the last
#              warehouse too (that partition receives no record at all); else
#              they use every warehouse
#   district   a handful of txns swap their first private access for a
#              NewOrder's DISTRICT access (a_nodist): three even ladder txns on
#              districts D0, D1, D2, three odd ones on D0, D0, D3 and one ONE
#              slot on D4, spread over the epoch and over the warehouses.
# Operands: payments 2^i where the epoch has at most 40 of them, i + 1 + salt
# otherwise; stock quantities 1 + (i + salt) % 10; link payments 2^20 + index.
# The rule (asserted by the builder): private rows are used once and a district
# has at most one writer outside the odd ladder txns, so under NO_WAIT /
# WAIT_DIE / OCC the ladder decides as adversarial's family 1 -- the k-th
# ladder txn commits iff k is even (an odd one meets the lock / the committed
# write on L_k; it leaves nothing behind, so its district access never blocks a
# later txn) -- and every other txn commits.  CALVIN: all commit; D0's three
# NewOrders take D_NEXT_O_ID + 1, + 2, + 3 in sequence order.
EMPTY, ONE = A.EMPTY, A.ONE
LINK_DIST = 10
MAX_TXN_ACC = 33


@functools.lru_cache(maxsize=None)
def ctx_world(world):
    return Ctx(num_wh=world)


def wh_to_part(w, world):
    return (w - 1) % world


def owner_bytes(cx, e, world):
    """the partition of every access, from the warehouse in its key
    (tpcc_helper.cpp:19-43 and wh_to_part); an ITEM read goes with the STOCK
    write that follows it (the supplying warehouse, as tpcc_gen.cpp has it)"""
    k, t = e.keys.astype(np.int64), e.tables
    cpd, mi = cx.kw["cust_per_dist"], cx.kw["max_items"]
    w = np.zeros(e.n_acc, np.int64)
    w[t == T_WH] = k[t == T_WH]
    w[t == T_DIST] = (k[t == T_DIST] - 1) // 10
    w[t == T_CUST] = ((k[t == T_CUST] - 1) // cpd - 1) // 10
    w[t == T_STOCK] = (k[t == T_STOCK] - 1) // mi
    assert not (t == T_CLAST).any(), "a last-name key does not name its warehouse"
    item = np.flatnonzero(t == T_ITEM)
    if item.size:
        assert item[-1] + 1 < e.n_acc and (t[item + 1] == T_STOCK).all() and (e.acc_txn()[item] == e.acc_txn()[item + 1]).all()
        w[item] = w[item + 1]
    assert e.n_acc == 0 or (w.min() >= 1 and w.max() <= cx.kw["num_wh"])
    return wh_to_part(w, world).astype(np.uint8)


def _spaced(c, m):
    """up to m of c, evenly spaced, first and last among them"""
    if len(c) <= m:
        return list(c)
    return [c[i] for i in sorted({round(j * (len(c) - 1) / (m - 1)) for j in range(m)})]


def ragged_tpcc_epoch(world, slots, own, salt=0):
    """(epoch with owner bytes, {cc: commit bytes}, info) -- the comment above"""
    cx = ctx_world(world)
    cpd, mi = cx.kw["cust_per_dist"], cx.kw["max_items"]
    slots = list(slots)
    lad = [i for i, s in enumerate(slots) if s is not EMPTY and s != ONE]
    ones = [i for i, s in enumerate(slots) if s is not EMPTY and s == ONE]
    assert all(2 + slots[i] <= MAX_TXN_ACC for i in lad)
    L = len(lad)
    narrow = own == "skip_last" and world >= 3
    link_wh = list(range(1, world if narrow else world + 1))
    priv_wh = {"spread": list(range(1, world + 1)), "part0": [1], "skip_last": list(range(1, max(2, world)))}[own]
    assert len(link_wh) >= 2

    def link(k):
        c = k // len(link_wh) + 1
        assert c <= cpd
        return cx.k_cust(c, LINK_DIST, link_wh[k % len(link_wh)])

    dist = [cx.k_dist(j % 9 + 1, link_wh[j % len(link_wh)]) for j in range(5)]
    padded = [k for k in range(L) if slots[lad[k]] >= 1]
    nod = {}  # slot -> district key
    for k, d in zip(_spaced([k for k in padded if k % 2 == 0], 3), (0, 1, 2)):
        nod[lad[k]] = dist[d]
    for k, d in zip(_spaced([k for k in padded if k % 2 == 1], 3), (0, 0, 3)):
        nod[lad[k]] = dist[d]
    if ones:
        nod[ones[len(ones) // 2]] = dist[4]
    # private accesses, in sequence order
    n_priv = sum((1 if s == ONE else s) for s in slots if s is not EMPTY) - len(nod)
    per_wh = {w: 0 for w in priv_wh}
    priv, n_cust = [], 0
    for i in range(n_priv):
        w = priv_wh[i % len(priv_wh)]
        j = per_wh[w]
        per_wh[w] += 1
        if j % 5 == 4:
            priv.append((T_STOCK, w, j // 5))
        else:
            priv.append((T_CUST, w, j - j // 5))
            n_cust += 1
    hs = _amounts(n_cust) if n_cust <= 40 else np.arange(n_cust, dtype=np.uint64) + np.uint64(1 + salt)
    b = _EB()
    pi = ci = si = 0
    sum_h = {False: 0, True: 0}  # payments' amounts: of the txns the deciders commit / of the others
    sum_q, n_q = {False: 0, True: 0}, {False: 0, True: 0}
    k = 0
    for i, s in enumerate(slots):
        if s is EMPTY:
            b.txn()
            continue
        acc, lost = [], False
        n = 1 if s == ONE else s
        if s != ONE:
            lost = k % 2 == 1
            for j, kk in enumerate((k, k + 1)):
                h = (1 << 20) + 2 * k + j
                acc.append(a_pcust(link(kk), h))
                sum_h[lost] += h
            k += 1
        if i in nod:
            acc.append(a_nodist(nod[i]))
            n -= 1
        for _ in range(n):
            t, w, j = priv[pi]
            pi += 1
            if t == T_STOCK:
                assert j < mi
                q = 1 + (si + salt) % 10
                si += 1
                acc.append(a_stock(cx.k_stock(j + 1, w), q))
                sum_q[lost] += q
                n_q[lost] += 1
            else:
                assert j < 9 * cpd
                h = int(hs[ci])
                ci += 1
                acc.append(a_pcust(cx.k_cust(j % cpd + 1, j // cpd + 1, w), h))
                sum_h[lost] += h
        b.txn(*acc)
    assert pi == n_priv and k == L
    e = b.epoch()
    e.owner = owner_bytes(cx, e, world)
    c = np.ones(len(slots), np.uint8)
    c[lad] = np.arange(L) % 2 == 0
    exp = {cc: c.copy() for cc in A.LOCKING + ("OCC",)}
    exp["CALVIN"] = np.ones(len(slots), np.uint8)
    # the rule's premises
    txn = e.acc_txn()
    is_link = (e.tables == T_CUST) & ((e.keys.astype(np.int64) - 1) // cpd % 10 == LINK_DIST % 10)
    is_dist = e.tables == T_DIST
    rest = ~(is_link | is_dist)
    pairs = e.tables[rest].astype(np.int64) << 40 | e.keys[rest].astype(np.int64)
    assert len(np.unique(pairs)) == int(rest.sum()), "a private row is used twice"
    assert int(is_link.sum()) == 2 * L and (e.types == WR).all()
    for kd in np.unique(e.keys[is_dist]):
        writers = txn[is_dist & (e.keys == kd)]
        assert len(np.unique(writers)) == len(writers) and int(c[writers].sum()) <= 1, "two committing NewOrders of a district"
    if L >= 2:
        lp = e.owner[is_link].reshape(L, 2)
        assert (lp[:, 0] != lp[:, 1]).all(), "consecutive links on one partition"
    info = dict(lad=np.array(lad, np.int64), nod=nod, dist=dist, sum_h=sum_h, sum_q=sum_q, n_q=n_q,
                n_cust=ci, n_link=2 * L, lost_pay=sum(1 for t in np.flatnonzero(c == 0) for a in
                                                   range(int(e.txn_begin[t]), int(e.txn_begin[t + 1]))
                                                   if e.tables[a] == T_CUST))
    return e, exp, info


def ragged_tpcc(world, epochs_slots, own):
    """A TCase of ragged_tpcc_epoch's epochs (salt: the epoch's number), run in
    order on one database."""
    cx = ctx_world(world)
    built_ = [ragged_tpcc_epoch(world, slots, own, salt=k) for k, slots in enumerate(epochs_slots)]
    epochs = [b[0] for b in built_]

    def applied(cc, k):
        return built_[k][1][cc]

    def closed(cc, k, before, after, oid):
        e, exp, info = built_[k]
        all_ = cc == "CALVIN"
        # payments: every applied one adds its amount to C_YTD_PAYMENT, takes it from C_BALANCE
        want = info["sum_h"][False] + (info["sum_h"][True] if all_ else 0)
        for col, sign in ((1, 1), (0, -1)):
            d = after[T_CUST][col].view(np.float64) - before[T_CUST][col].view(np.float64)
            assert (d == np.round(d)).all() and int(d.astype(np.int64).sum()) == sign * want
        pays = info["n_cust"] + info["n_link"] - (0 if all_ else info["lost_pay"])
        grown = after[T_CUST][2].view(np.float64) - before[T_CUST][2].view(np.float64)
        assert int(np.round(grown).sum()) == pays
        # stock: one write a row
        sq = info["sum_q"][False] + (info["sum_q"][True] if all_ else 0)
        nq = info["n_q"][False] + (info["n_q"][True] if all_ else 0)
        assert int((after[T_STOCK][1].view(np.int64) - before[T_STOCK][1].view(np.int64)).sum()) == sq
        assert int((after[T_STOCK][2] != before[T_STOCK][2]).sum()) == nq
        assert int((after[T_STOCK][2].view(np.int64) - before[T_STOCK][2].view(np.int64)).sum()) == nq
        # districts: the committing NewOrder takes D_NEXT_O_ID + 1; under CALVIN all of them, in sequence order
        by_d = {}
        for slot in sorted(info["nod"]):
            by_d.setdefault(info["nod"][slot], []).append(slot)
        c = exp[cc]
        took = 0
        for kd, txns in by_d.items():
            r = int(cx.row(T_DIST, kd))
            first = int(before[T_DIST][1][r])
            ap = [t for t in txns if c[t]]
            assert [int(oid[t]) for t in ap] == list(range(first + 1, first + 1 + len(ap)))
            assert int(after[T_DIST][1][r]) == first + len(ap) and (all_ or len(ap) <= 1)
            took += len(ap)
        assert int((oid != 0).sum()) == took
        assert all(np.array_equal(after[t][col], before[t][col]) for t in (T_WH, T_ITEM) for col in range(3))

    return TCase(cx, epochs, applied, closed, extra=dict(world=world, own=own, info=[b[2] for b in built_]))


# ---- the cuts of a TpccEpoch (adversarial.contiguous_chunks / strided_chunks
# / trim_tail, carrying tables, args and owner)
def _take(e, ids):
    tb = e.txn_begin.astype(np.int64)
    lens = np.diff(tb)[ids]
    ltb = np.zeros(len(ids) + 1, np.int64)
    ltb[1:] = np.cumsum(lens)
    idx = np.repeat(tb[ids] - ltb[:-1], lens) + np.arange(int(ltb[-1]))
    return T.TpccEpoch(e.keys[idx].copy(), e.types[idx].copy(), ltb.astype(np.uint32), e.tables[idx].copy(),
                       e.args[idx].copy(), None, None if e.owner is None else e.owner[idx].copy())


def contiguous_chunks(e, world):
    tpr = (e.n_txn + world - 1) // world
    return [_take(e, np.arange(min(r * tpr, e.n_txn), min((r + 1) * tpr, e.n_txn))) for r in range(world)], tpr


def strided_chunks(e, world):
    tpr = (e.n_txn + world - 1) // world
    return [_take(e, np.arange(q, e.n_txn, world)) for q in range(world)], tpr


def trim_tail(b):
    n = np.flatnonzero(np.diff(b.txn_begin.astype(np.int64)))
    return T.TpccEpoch(b.keys, b.types, b.txn_begin[:(int(n[-1]) + 2) if n.size else 1].copy(), b.tables, b.args,
                       None, b.owner)


def cut(e, world, order):
    """the origins' batches of global epoch `e` (trailing empty txns dropped)
    and txns_per_rank"""
    parts, tpr = strided_chunks(e, world) if order == "position" else contiguous_chunks(e, world)
    return [trim_tail(p) for p in parts], tpr


def padded(e, n_txn):
    """`e` with empty txns appended up to n_txn: the epoch the partitioned run
    decides when the origins' slots outnumber the txns"""
    tb = np.concatenate([e.txn_begin, np.full(n_txn - e.n_txn, e.txn_begin[-1], np.uint32)])
    return T.TpccEpoch(e.keys, e.types, tb, e.tables, e.args, None, e.owner)


# ---- family 8's shapes (per-origin slot lists through adversarial.arrange)
PART_WORLDS = (2, 3)
PART_SHAPES = ("edges", "mix")
MIX_TPR = 37


def _tsegment(total):
    """one origin's batch of `total` accesses in ladder txns of 31; where it
    spans more than a tile, a txn of 33 accesses sits across the first edge"""
    X = A.structural_constants()["kOwnerTile"]
    if total < X + MAX_TXN_ACC:
        return A._fill(total, 31)
    return A._fill(X - 16, 31) + [MAX_TXN_ACC - 2] + A._fill(total - X - 17, 31)


def part_sizes():
    X = A.structural_constants()["kOwnerTile"]
    return [X - 1, X, X + 1, 2 * X + 1]


SMALL_BATCH = [0, ONE, 3, EMPTY, 31, 1, EMPTY, ONE, 12]


def part_slots(shape, world, order):
    """(slot lists of the shape's epochs in sequence order, txns_per_rank)
      edges  four epochs: one origin hands over kTile - 1, kTile, kTile + 1,
             2 * kTile + 1 accesses in turn (the owner split's tile), the
             origin before it nothing at all, a third a small batch
      mix    two epochs of MIX_TPR txns an origin (neither a multiple of
             world nor of 64) mixing 0-, 1-, 2-, ... 33-access txns"""
    if shape == "edges":
        per_epoch = []
        for k, size in enumerate(part_sizes()):
            per = [list(SMALL_BATCH) for _ in range(world)]
            per[k % world] = []
            per[(k + 1) % world] = _tsegment(size)
            per_epoch.append(per)
        tpr = max(len(s) for per in per_epoch for s in per)
        return [A.arrange(per, order, tpr) for per in per_epoch], tpr
    assert shape == "mix" and MIX_TPR % world and MIX_TPR % 64
    pat = [EMPTY, 31, ONE, 0, EMPTY, 0, 31, 7, ONE, 12, 1]
    return [[pat[(i + 3 * k) % len(pat)] for i in range(MIX_TPR * world)] for k in range(2)], MIX_TPR


@functools.lru_cache(maxsize=None)
def part_case(shape, world, own, order):
    slots, tpr = part_slots(shape, world, order)
    case = ragged_tpcc(world, slots, own)
    case.extra.update(tpr=tpr, order=order, shape=shape)
    return case
