"""Exponential back-off in the device closed loop (dv_closed_loop_backoff):
the numpy model of the ring -- the specification -- and the CPU checks: the
model at D = 1 against the plain loop, conservation, the slot bound, the
struct's layout, the entry point's refusals and the statistics line.

The rule (include/dvcc.h): a ring of D slots of parked txns (src, born,
aborts).  After epoch k is decided each aborted txn, in sequence order, with
a = aborts + 1, is appended to slot (k + min(2^(a-1), D)) % D.  Epoch k + 1
is then the first R = min(c, n_txn) of the c entries of slot (k + 1) % D, the
other c - R (the spill) moving to the tail of slot (k + 2) % D, then
n_txn - R fresh pool txns from the cursor.  A released txn's accesses are
those of pool txn src.  The model is driven by the oracle's commit bytes,
never by the engine's.
"""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import _oracle as O
import dvcc
from dvcc import Epoch, stats
from dvcc import _lib as L
from test_carry import ORACLE_CC, _gather_txns, _pool, host_closed_loop
from test_loop_track import CF_N, CF_POOL, TrackModel, closed_form_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 1 << 13


def slot_bound(n_txn, D):
    """no slot ever holds more: n (D + log2 D)"""
    return n_txn * (D + D.bit_length() - 1)


class BackoffModel:
    """The ring, the epochs' identities and abort counts, and what the tracker
    and the counters record.  build() makes the next epoch (the release step);
    epoch(commit) logs and parks the epoch just decided and builds the next."""

    def __init__(self, pool_n, cur, n_txn, D, n_bins=64, first_epoch=0, slot_cap=None):
        assert D in (1, 2, 4, 8, 16)
        self.pool_n, self.cur, self.n_txn, self.D, self.n_bins = pool_n, cur, n_txn, D, n_bins
        self.lgD = D.bit_length() - 1
        self.slot_cap = slot_cap if slot_cap is not None else slot_bound(n_txn, D)
        self.k = first_epoch  # the epoch built last / decided next
        self.slots = [self._none() for _ in range(D)]
        self.ep = None        # (src, born, aborts) of epoch self.k
        self.seen = {}
        self.drawn = []       # identity words of every fresh txn
        self.log, self.epoch_end, self.pos = [], [], 0
        self.hist = np.zeros(n_bins, np.int64)
        self.totals = [0, 0, 0, 0]  # committed, aborted, first aborts, most aborts at a commit
        self.spilled = self.lost = self.wait = 0
        self.fullest = 0

    @staticmethod
    def _none():
        return tuple(np.zeros(0, np.int64) for _ in range(3))

    def _append(self, slot, items):
        """entries at positions >= slot_cap are counted and not written"""
        have = len(self.slots[slot][0])
        room = max(0, self.slot_cap - have)
        self.lost += max(0, len(items[0]) - room)
        self.slots[slot] = tuple(np.concatenate([a, b[:room]]) for a, b in zip(self.slots[slot], items))
        self.fullest = max(self.fullest, len(self.slots[slot][0]))

    def build(self):
        """epoch self.k from slot k % D and the pool"""
        e, D, n = self.k, self.D, self.n_txn
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
        self.ep = (np.concatenate([ent[0][:R], fs]), np.concatenate([ent[1][:R], fb]),
                   np.concatenate([ent[2][:R], np.zeros(F, np.int64)]))
        self.released = R
        return self.ep

    def epoch(self, commit):
        k = self.k
        src, born, ab = self.ep
        self.seen[k] = self.ep
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
        cls = np.minimum(a - 1, self.lgD)  # delay min(2^(a-1), D) = 2^cls
        for c in range(self.lgD + 1):
            m = cls == c
            self._append((k + (1 << c)) % self.D, (src[~cm][m], born[~cm][m], a[m]))
        self.k = k + 1
        return self.build()

    def drain(self):
        self.log, self.epoch_end, self.pos = [], [], 0

    def parked_now(self):
        return sum(len(s[0]) for s in self.slots)

    def words(self, k):
        src, born, _ = self.ep if k == self.k else self.seen[k]
        return src | born << 32

    def aborts_of(self, k):
        return (self.ep if k == self.k else self.seen[k])[2].astype(np.uint8)

    def counters(self):
        return [self.spilled, self.lost, self.wait, self.parked_now()]

    def log_words(self):
        return np.concatenate([s | b << 32 for s, b in self.log]) if self.log else np.zeros(0, np.int64)


def host_epoch(pool, src):
    """the epoch whose txn t holds the accesses of pool txn src[t]"""
    idx, ntb = _gather_txns(pool.txn_begin.astype(np.int64), np.asarray(src, np.int64))
    return Epoch(pool.keys[idx].copy(), pool.types[idx].copy(), ntb)


def host_backoff_loop(cc, tab, f0, pool, cur, n_txn, n_epochs, D, **kw):
    """the oracle's loop under the model: per epoch (commit bytes, stats, the
    host epoch), the epoch left, and the model"""
    m = BackoffModel(pool.n_txn, cur, n_txn, D, **kw)
    host = host_epoch(pool, m.build()[0])
    out = []
    for _ in range(n_epochs):
        c_ref, _, st_ref = O.epoch_run(ORACLE_CC[cc], tab.ix, f0, host.n_txn, host.txn_begin, host.keys, host.types)
        out.append((c_ref[:host.n_txn].copy(), st_ref, host))
        host = host_epoch(pool, m.epoch(c_ref)[0])
    return out, host, m


_cache = {}


def ref_backoff(cc, pool_key, n_txn, n_epochs, cur0, D, rows=ROWS, **kw):
    """computed once per shape, read-only afterwards: (pool, ref, next epoch, model, final table)"""
    key = (cc, pool_key, n_txn, n_epochs, cur0, D, rows, tuple(sorted(kw.items())))
    if key not in _cache:
        pool = closed_form_pool() if pool_key == "closed form" else _pool(rows, *pool_key)
        tab = O.YcsbTable(rows)
        f0 = tab.f0.copy()
        ref, nxt, m = host_backoff_loop(cc, tab, f0, pool, cur0, n_txn, n_epochs, D, **kw)
        _cache[key] = (pool, ref, nxt, m, f0)
    return _cache[key]


def check_conservation(m):
    """every txn drawn is in the epoch, in exactly one slot, or in the log"""
    held = [m.ep[0] | m.ep[1] << 32] + [s[0] | s[1] << 32 for s in m.slots] + [m.log_words()]
    held = np.sort(np.concatenate(held))
    drawn = np.sort(np.concatenate(m.drawn))
    assert len(np.unique(drawn)) == len(drawn)
    assert np.array_equal(held, drawn)


N, E, POOL_KEY = 2000, 24, (20000, 3)


def test_d1_is_the_plain_loop():
    """D = 1 against TrackModel and host_closed_loop: epochs, commit bytes,
    cursor, table, log, histogram, totals"""
    for cc in (dvcc.NO_WAIT, dvcc.OCC):
        pool, ref, nxt, m, f0 = ref_backoff(cc, POOL_KEY, N, E, 0, 1)
        tab = O.YcsbTable(ROWS)
        g0 = tab.f0.copy()
        plain, pnxt, pcur = host_closed_loop(cc, tab, g0, pool, 0, N, E)
        t = TrackModel(pool.n_txn, 0, N)
        for (c, _, h), (pc, _, ph) in zip(ref, plain):
            assert np.array_equal(c, pc) and np.array_equal(h.keys, ph.keys)
            assert np.array_equal(h.txn_begin, ph.txn_begin) and np.array_equal(h.types, ph.types)
            t.epoch(pc)
        assert m.cur == pcur == t.cur and np.array_equal(f0, g0)
        assert np.array_equal(nxt.keys, pnxt.keys) and np.array_equal(nxt.txn_begin, pnxt.txn_begin)
        assert m.epoch_end == t.epoch_end and m.totals == t.totals and np.array_equal(m.hist, t.hist)
        assert np.array_equal(m.log_words(), t.log_words())
        assert np.array_equal(m.words(E), t.words(E)) and np.array_equal(m.words(E - 1), t.words(E - 1))
        assert np.array_equal(m.aborts_of(E), E - (m.words(E) >> 32))  # an abort per epoch since birth
        assert m.spilled == 0 and m.lost == 0 and m.fullest <= N
        assert m.wait == int((t.hist * np.arange(t.n_bins)).sum())
        check_conservation(m)


@pytest.mark.parametrize("D", [2, 4, 8, 16])
def test_conservation_and_the_slot_bound(D):
    commits = {}
    for cc in (dvcc.NO_WAIT, dvcc.OCC):
        pool, ref, nxt, m, f0 = ref_backoff(cc, POOL_KEY, N, E, 0, D)
        check_conservation(m)
        assert m.lost == 0 and 0 < m.fullest <= slot_bound(N, D)
        assert m.totals[3] >= 1 and m.wait >= m.totals[3]
        assert m.totals[0] + m.totals[1] == N * E and m.epoch_end[-1] == m.totals[0]
        # a txn with a aborts has waited 1 + 2 + .. capped delays at least
        src, born, ab = m.ep
        d = np.minimum(1 << np.minimum(np.maximum(ab - 1, 0), 5), D)
        assert ((E - born >= ab) & ((ab == 0) | (E - born >= d))).all()
        commits[cc] = m.totals[0]
    plain = ref_backoff(dvcc.NO_WAIT, POOL_KEY, N, E, 0, 1)[3].totals[0]
    assert commits[dvcc.NO_WAIT] > plain  # scheduling alone: more commits in the same epochs
    if D <= 8:
        assert ref_backoff(dvcc.NO_WAIT, POOL_KEY, N, E, 0, D)[3].spilled > 0


@pytest.mark.parametrize("D", [2, 8])
def test_closed_form_spills(D):
    """300 txns, each one write of key 1: one commit per epoch, everything else
    backs off, and the slots overflow into their successors"""
    pool, ref, nxt, m, f0 = ref_backoff(dvcc.NO_WAIT, "closed form", CF_N, 40, 0, D, rows=16)
    assert all(int(c.sum()) == 1 and c[0] == 1 for c, _, _ in ref)
    assert m.spilled > 0 and m.lost == 0 and m.fullest <= slot_bound(CF_N, D)
    assert m.cur == (sum(len(d) for d in m.drawn)) % CF_POOL
    check_conservation(m)


def test_a_small_slot_cap_loses_entries():
    full = ref_backoff(dvcc.NO_WAIT, "closed form", CF_N, 40, 0, 2, rows=16)[3]
    assert full.fullest > 300
    m = ref_backoff(dvcc.NO_WAIT, "closed form", CF_N, 40, 0, 2, rows=16, slot_cap=300)[3]
    assert m.lost > 0 and m.fullest == 300
    assert len(np.concatenate(m.drawn)) == m.lost + CF_N + m.parked_now() + m.pos


def test_retry_summary_fields_with_wait_epochs():
    hist, totals = [5, 3, 2], [10, 9, 6, 2]
    sts = [SimpleNamespace(committed=5, aborted=5, n_txn=10, write_cnt=5) for _ in range(2)]
    plain = dict(stats.retry_summary_fields(2.0, sts, totals, hist, 1))
    assert abs(plain["txn_run_time"] - (5 * 1 + 3 * 2 + 2 * 3) * 1.0) < 1e-12  # (unchanged without wait_epochs)
    assert plain == dict(stats.retry_summary_fields(2.0, sts, totals, hist, 1, wait_epochs=None))
    # under back-off the three commits after one abort waited 1 epoch, the two after two 1 + 2
    got = dict(stats.retry_summary_fields(2.0, sts, totals, hist, 1, wait_epochs=3 * 1 + 2 * 3))
    assert abs(got["txn_run_time"] - (9 + 10) * 1.0) < 1e-12
    assert abs(got["txn_run_avg_time"] - 1.9) < 1e-12
    assert got["unique_txn_abort_cnt"] == 6
    for k in plain:
        if k not in ("txn_run_time", "txn_run_avg_time"):
            assert got[k] == plain[k], k


def _desc(**kw):
    """a well-formed dv_loop_backoff over made-up addresses (never
    dereferenced by the attach call), with fields overridden"""
    ab = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    d = dict(n_slots=4, slot_cap=100, park_ids=0x3000, park_aborts=0x4000, slot_count=0x5000, aborts=ab,
             counters=0x6000)
    d.update(kw)
    return L.LoopBackoffDesc(d["n_slots"], d["slot_cap"], d["park_ids"], d["park_aborts"], d["slot_count"],
                             d["aborts"], d["counters"])


def malformed_descs():
    """(name, struct): each refused with DV_ERR_ARG at attach time"""
    null_ab = (ctypes.c_void_p * 2)(0x1000, None)
    return [("n_slots 0", _desc(n_slots=0)), ("n_slots 3", _desc(n_slots=3)), ("n_slots 32", _desc(n_slots=32)),
            ("slot_cap", _desc(slot_cap=0)), ("park_ids", _desc(park_ids=None)),
            ("park_aborts", _desc(park_aborts=None)), ("slot_count", _desc(slot_count=None)),
            ("aborts", _desc(aborts=None)), ("aborts entry", _desc(aborts=null_ab)),
            ("counters", _desc(counters=None))]


def test_backoff_entry_refuses_a_null_context():
    f = L.lib().dv_closed_loop_backoff
    assert f(None, None) == L.DV_ERR_ARG
    assert f(None, ctypes.byref(_desc())) == L.DV_ERR_ARG
    for name, d in malformed_descs():
        assert f(None, ctypes.byref(d)) == L.DV_ERR_ARG, name


def test_loop_backoff_layout_matches_the_header(tmp_path):
    """the ctypes mirror of dv_loop_backoff against the header, compiled by gcc"""
    name, cls = "dv_loop_backoff", L.LoopBackoffDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dvcc.h"', "int main(void) {",
             f'printf("{name} %zu\\n", sizeof({name}));']
    for f, _ in cls._fields_:
        lines.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines.append("return 0; }")
    src, exe = tmp_path / "sz.c", tmp_path / "sz"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got[name]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, f
    assert ("dv_closed_loop_backoff", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(cls)]) in L.SIGNATURES
