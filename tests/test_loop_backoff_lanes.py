"""Exponential back-off in the closed loop over decision lanes
(dv_closed_loop_backoff_lanes): the numpy model of the shared ring -- the
specification -- and the CPU checks: the model at D = 1 against the plain
lanes loop and its tracker, conservation, the slot bound, the closed form's
spill, a small slot_cap, the header and the entry point's refusals.

The rule (include/dvcc.h): tests/test_loop_backoff.py's, with one change -- an
abort of epoch k cannot return before epoch k + L (L lanes).  After epoch k is
decided each aborted txn, in sequence order, with a = aborts + 1, is appended
to slot (k + L - 1 + min(2^(a-1), D)) % D.  Epoch e = k + L is then the first
R = min(c, n_txn) of the c entries of slot e % D, the other c - R (the spill)
moving to the tail of slot (e + 1) % D, then n_txn - R fresh pool txns from
the shared cursor.  A call's first L epochs are built by the same release with
no park before it.  The model is driven by the oracle's commit bytes, never
by the engine's.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import _oracle as O
import dvcc
from dvcc import _lib as L
from test_carry import ORACLE_CC, _pool, host_closed_loop_lanes
from test_loop_backoff import (ROWS, BackoffModel, _desc, check_conservation, host_epoch, malformed_descs,
                               slot_bound)
from test_loop_track import CF_N, CF_POOL, TrackModel, closed_form_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LANES = 8


class LanesBackoffModel(BackoffModel):
    """BackoffModel over L lanes: L epochs are built and undecided at any time
    (self.eps: epoch number -> (src, born, aborts)); self.k is the epoch
    decided next, self.e the epoch built next.  start() builds a call's first
    L epochs; epoch(commit) logs and parks epoch k and builds epoch k + L."""

    def __init__(self, pool_n, cur, n_txn, D, lanes, **kw):
        self.eps = {}
        super().__init__(pool_n, cur, n_txn, D, **kw)
        self.L = lanes
        self.e = self.k
        self.classes = set()  # the delay classes parked so far

    # (check_conservation's "the epoch": every epoch built and not yet decided)
    @property
    def ep(self):
        return tuple(np.concatenate([self.eps[e][i] for e in sorted(self.eps)]) for i in range(3))

    @ep.setter
    def ep(self, v):
        pass

    def build(self):
        """epoch self.e from slot e % D and the pool"""
        e, D, n = self.e, self.D, self.n_txn
        s = e % D
        ent = self.slots[s]
        R = min(len(ent[0]), n)
        spill = tuple(a[R:] for a in ent)
        self.slots[s] = self._none()
        self.spilled += len(spill[0])
        if len(spill[0]):
            assert D > 1, "D = 1 never spills"
            self._append((e + 1) % D, spill)
        F = n - R
        fs = (self.cur + np.arange(F, dtype=np.int64)) % self.pool_n
        self.cur = (self.cur + F) % self.pool_n
        fb = np.full(F, e, np.int64)
        self.drawn.append(fs | fb << 32)
        self.eps[e] = (np.concatenate([ent[0][:R], fs]), np.concatenate([ent[1][:R], fb]),
                       np.concatenate([ent[2][:R], np.zeros(F, np.int64)]))
        self.released = R
        self.e = e + 1
        return self.eps[e]

    def start(self):
        """a call without resume: its first L epochs, lane 0 first"""
        return [self.build() for _ in range(self.L)]

    def epoch(self, commit):
        k = self.k
        assert self.e == k + self.L
        src, born, ab = self.seen[k] = self.eps.pop(k)
        cm = np.asarray(commit[:self.n_txn]) != 0
        self.log.append((src[cm], born[cm]))
        self.pos += int(cm.sum())
        self.epoch_end.append(self.pos)
        np.add.at(self.hist, np.minimum(ab[cm], self.n_bins - 1), 1)
        self.totals[0] += int(cm.sum())
        self.totals[1] += int((~cm).sum())
        self.totals[2] += int((ab[~cm] == 0).sum())
        if cm.any():
            self.totals[3] = max(self.totals[3], int(ab[cm].max()))
        self.wait += int((k - born[cm]).sum())
        a = np.minimum(ab[~cm] + 1, 255)
        cls = np.minimum(a - 1, self.lgD)  # delay L - 1 + min(2^(a-1), D) = L - 1 + 2^cls
        for c in range(self.lgD + 1):
            m = cls == c
            if m.any():
                self.classes.add(c)
            self._append((k + self.L - 1 + (1 << c)) % self.D, (src[~cm][m], born[~cm][m], a[m]))
        self.k = k + 1
        return self.build()

    def words(self, k):
        src, born, _ = self.eps[k] if k in self.eps else self.seen[k]
        return src | born << 32

    def aborts_of(self, k):
        return (self.eps[k] if k in self.eps else self.seen[k])[2].astype(np.uint8)


def host_backoff_lanes_loop(cc, tab, f0, pool, cur, n_txn, n_epochs, D, lanes, **kw):
    """the oracle's lanes loop under the model: per epoch (commit bytes, stats,
    the host epoch), the L epochs left (by number), and the model"""
    m = LanesBackoffModel(pool.n_txn, cur, n_txn, D, lanes, **kw)
    hosts = {e: host_epoch(pool, ep[0]) for e, ep in enumerate(m.start())}
    out = []
    for k in range(n_epochs):
        host = hosts.pop(k)
        c_ref, _, st_ref = O.epoch_run(ORACLE_CC[cc], tab.ix, f0, host.n_txn, host.txn_begin, host.keys, host.types)
        out.append((c_ref[:host.n_txn].copy(), st_ref, host))
        hosts[k + lanes] = host_epoch(pool, m.epoch(c_ref)[0])
    return out, hosts, m


_cache = {}


def ref_backoff_lanes(cc, pool_key, n_txn, n_epochs, D, lanes, rows=ROWS, **kw):
    """computed once per shape, read-only afterwards: (pool, ref, epochs left, model, final table)"""
    key = (cc, pool_key, n_txn, n_epochs, D, lanes, rows, tuple(sorted(kw.items())))
    if key not in _cache:
        pool = closed_form_pool() if pool_key == "closed form" else _pool(rows, *pool_key)
        tab = O.YcsbTable(rows)
        f0 = tab.f0.copy()
        ref, nxt, m = host_backoff_lanes_loop(cc, tab, f0, pool, 0, n_txn, n_epochs, D, lanes, **kw)
        _cache[key] = (pool, ref, nxt, m, f0)
    return _cache[key]


N, POOL_KEY = 2000, (20000, 3)
# D = 16: the epochs (a multiple of 2 L) after which the model shows class 4 --
# a txn parked with five aborts -- chosen on the CPU: 6 L epochs show none
E16 = {2: 20, 3: 24, 4: 32}


@pytest.mark.parametrize("lanes", [2, 3, 4])
def test_d1_is_the_plain_lanes_loop(lanes):
    """D = 1 against host_closed_loop_lanes and TrackModel: epochs, commit
    bytes, the epochs left, cursor, table, log, histogram, totals"""
    E = 6 * lanes
    for cc in (dvcc.NO_WAIT, dvcc.OCC):
        pool, ref, nxt, m, f0 = ref_backoff_lanes(cc, POOL_KEY, N, E, 1, lanes)
        tab = O.YcsbTable(ROWS)
        g0 = tab.f0.copy()
        plain, pnxt, pcur = host_closed_loop_lanes(cc, tab, g0, pool, 0, N, E, lanes)
        t = TrackModel(pool.n_txn, 0, N, lanes=lanes)
        for (c, _, h), (pc, _, ph) in zip(ref, plain):
            assert np.array_equal(c, pc) and np.array_equal(h.keys, ph.keys)
            assert np.array_equal(h.txn_begin, ph.txn_begin) and np.array_equal(h.types, ph.types)
            t.epoch(pc)
        assert m.cur == pcur == t.cur and np.array_equal(f0, g0)
        assert sorted(nxt) == sorted(pnxt) == list(range(E, E + lanes))
        for e in nxt:
            assert np.array_equal(nxt[e].keys, pnxt[e].keys) and np.array_equal(nxt[e].txn_begin, pnxt[e].txn_begin)
            assert np.array_equal(m.words(e), t.words(e))
            assert np.array_equal(m.aborts_of(e) * lanes, e - (m.words(e) >> 32))  # an abort per L epochs
        assert np.array_equal(m.words(E - 1), t.words(E - 1))
        assert m.epoch_end == t.epoch_end and m.totals == t.totals and np.array_equal(m.hist, t.hist)
        assert np.array_equal(m.log_words(), t.log_words())
        assert m.spilled == 0 and m.lost == 0 and m.fullest <= N
        assert m.wait == lanes * int((t.hist * np.arange(t.n_bins)).sum())
        check_conservation(m)


@pytest.mark.parametrize("lanes", [2, 3, 4])
@pytest.mark.parametrize("D", [2, 4, 8, 16])
def test_conservation_and_the_slot_bound(D, lanes):
    E = 6 * lanes
    commits = {}
    for cc in (dvcc.NO_WAIT, dvcc.OCC):
        pool, ref, nxt, m, f0 = ref_backoff_lanes(cc, POOL_KEY, N, E, D, lanes)
        check_conservation(m)
        assert m.lost == 0 and 0 < m.fullest <= slot_bound(N, D)
        assert m.spilled > 0
        assert m.classes >= set(range(min(m.lgD, 3) + 1))
        assert m.totals[3] >= 1 and m.wait >= m.totals[3]
        assert m.totals[0] + m.totals[1] == N * E and m.epoch_end[-1] == m.totals[0]
        # a txn with a aborts has waited a (L - 1) epochs and 1 + 2 + .. capped delays at least
        for e, (src, born, ab) in m.eps.items():
            d = np.minimum(1 << np.minimum(np.maximum(ab - 1, 0), 5), D)
            assert ((e - born >= ab * lanes) & ((ab == 0) | (e - born >= lanes - 1 + d))).all()
        commits[cc] = m.totals[0]
    plain = ref_backoff_lanes(dvcc.NO_WAIT, POOL_KEY, N, E, 1, lanes)[3].totals[0]
    assert commits[dvcc.NO_WAIT] > plain  # scheduling alone: more commits in the same epochs


@pytest.mark.parametrize("lanes", [2, 3, 4])
def test_d16_reaches_class_4(lanes):
    """6 L epochs show no fifth abort; E16[L] epochs (a multiple of 2 L) do"""
    short = ref_backoff_lanes(dvcc.NO_WAIT, POOL_KEY, N, 6 * lanes, 16, lanes)[3]
    assert 4 not in short.classes
    E = E16[lanes]
    assert E % (2 * lanes) == 0
    m = ref_backoff_lanes(dvcc.NO_WAIT, POOL_KEY, N, E, 16, lanes)[3]
    assert m.classes == {0, 1, 2, 3, 4} and m.lost == 0 and m.spilled > 0
    assert any((s[2] >= 5).any() for s in m.slots) or any((ep[2] >= 5).any() for ep in m.eps.values())
    check_conservation(m)


@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("D", [2, 8])
def test_closed_form_spills(D, lanes):
    """300 txns, each one write of key 1: one commit per epoch, everything else
    backs off, and the slots overflow into their successors"""
    pool, ref, nxt, m, f0 = ref_backoff_lanes(dvcc.NO_WAIT, "closed form", CF_N, 40, D, lanes, rows=16)
    assert all(int(c.sum()) == 1 and c[0] == 1 for c, _, _ in ref)
    assert m.spilled > 0 and m.lost == 0 and m.fullest <= slot_bound(CF_N, D)
    assert m.cur == (sum(len(d) for d in m.drawn)) % CF_POOL
    check_conservation(m)


def test_a_small_slot_cap_loses_entries():
    full = ref_backoff_lanes(dvcc.NO_WAIT, "closed form", CF_N, 40, 2, 2, rows=16)[3]
    assert full.fullest > 300
    m = ref_backoff_lanes(dvcc.NO_WAIT, "closed form", CF_N, 40, 2, 2, rows=16, slot_cap=300)[3]
    assert m.lost > 0 and m.fullest == 300
    assert len(np.concatenate(m.drawn)) == m.lost + 2 * CF_N + m.parked_now() + m.pos


def test_the_header_declares_the_entry():
    text = open(os.path.join(ROOT, "include", "dvcc.h")).read()
    assert re.search(r"int\s+dv_closed_loop_backoff_lanes\s*\(\s*dv_ctx\s*\*\s*ctx\s*,\s*const\s+dv_loop_backoff\s*\*"
                     r"\s*bo\s*,\s*uint32_t\s+n_lanes\s*\)\s*;", text)
    sig = ("dv_closed_loop_backoff_lanes", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(L.LoopBackoffDesc),
                                                           ctypes.c_uint32])
    assert sig in L.SIGNATURES


def test_lanes_entry_refuses_a_null_context_and_no_lanes():
    f = L.lib().dv_closed_loop_backoff_lanes
    for n_lanes in (0, 1, 2, MAX_LANES, MAX_LANES + 1):
        assert f(None, None, n_lanes) == L.DV_ERR_ARG
        assert f(None, ctypes.byref(_desc()), n_lanes) == L.DV_ERR_ARG
    for name, d in malformed_descs():
        assert f(None, ctypes.byref(d), 2) == L.DV_ERR_ARG, name
