"""Identity through the device closed loop (dv_closed_loop_track): the numpy
model of the tracker, and the CPU checks -- the entry point's refusals, the
struct's layout, the model against a closed form and the statistics line.

The model restates the rule beside tests/test_carry.py's host loops: every
epoch carries a (src, born) pair per txn; the carried txns' pairs are
ids[commit == 0] in order, the fresh ones (cur + arange(F)) % pool_n with the
number of the epoch being built, and epoch k's log slice is ids[commit == 1].
Its commit bytes come from the oracle, never from the engine
(tests/test_loop_track_gpu.py drives it from host_closed_loop's epochs).
"""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np

import _oracle as O
import dvcc
from dvcc import Epoch, stats
from dvcc import _lib as L
from test_carry import host_closed_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TrackModel:
    """The tracker of a closed loop over `lanes` interleaved loops (1: the
    single loops): epoch k + lanes is epoch k's aborted txns then fresh pool
    txns, the cursor shared in epoch order.  epoch(commit) logs the next
    epoch in order."""

    def __init__(self, pool_n, cur, n_txn, lanes=1, n_bins=64, first_epoch=0, log_cap=None):
        self.pool_n, self.cur, self.n_txn, self.L, self.n_bins = pool_n, cur, n_txn, lanes, n_bins
        self.k = first_epoch
        self.ids = {}  # epoch number -> (src, born) of its txns
        self.seen = {}  # ... of the epochs already run
        for ln in range(lanes):
            self.ids[first_epoch + ln] = self._fresh(n_txn, first_epoch + ln)
        self.log = []        # per epoch: (src, born) of its commits, in sequence order
        self.epoch_end = []  # the commit count after each epoch
        self.pos = 0
        self.hist = np.zeros(n_bins, np.int64)
        self.totals = [0, 0, 0, 0]  # committed, aborted, first aborts, max retries at commit
        self.log_cap = log_cap

    def _fresh(self, n, born):
        src = (self.cur + np.arange(n, dtype=np.int64)) % self.pool_n
        self.cur = (self.cur + n) % self.pool_n
        return src, np.full(n, born, np.int64)

    def epoch(self, commit):
        k = self.k
        src, born = self.ids.pop(k)
        self.seen[k] = (src, born)
        cm = np.asarray(commit[:self.n_txn]) != 0
        assert ((k - born) % self.L == 0).all()  # a txn returns L epochs later: the division is exact
        retries = (k - born[cm]) // self.L
        self.log.append((src[cm], born[cm]))
        self.pos += int(cm.sum())
        self.epoch_end.append(self.pos)
        np.add.at(self.hist, np.minimum(retries, self.n_bins - 1), 1)
        self.totals[0] += int(cm.sum())
        self.totals[1] += int((~cm).sum())
        self.totals[2] += int((born[~cm] == k).sum())
        if len(retries):
            self.totals[3] = max(self.totals[3], int(retries.max()))
        fs, fb = self._fresh(int(cm.sum()), k + self.L)
        self.ids[k + self.L] = (np.concatenate([src[~cm], fs]), np.concatenate([born[~cm], fb]))
        self.k = k + 1

    def drain(self):
        self.log, self.epoch_end, self.pos = [], [], 0

    def words(self, k):
        """the identity words of epoch k as the device holds them"""
        src, born = self.ids[k] if k in self.ids else self.seen[k]
        return src | born << 32

    def log_words(self):
        """the whole log, cut at log_cap"""
        w = np.concatenate([s | b << 32 for s, b in self.log]) if self.log else np.zeros(0, np.int64)
        return w if self.log_cap is None else w[:self.log_cap]


# ---- the closed form: every pool txn is one write of key 1 -------------------
# NO_WAIT grants the row to the first txn in sequence order and aborts every
# other one, so exactly one txn commits per epoch: the head of the queue.
# Epoch 0 holds pool txns 0 .. N-1 (born 0); epoch k >= 1 is epoch k-1 without
# its head, plus one fresh txn, pool txn N-1+k, born k.  Hence
#   epoch k commits src = k, born = max(0, k - N + 1), after min(k, N - 1) retries;
#   aborted      = E (N - 1)              (N - 1 per epoch)
#   first aborts = (N - 1) + (E - 1)      (epoch 0: all but its head; then the one fresh txn)
#   histogram    : with m = min(B - 1, N - 1), the last bin any commit reaches (B bins),
#                  bin r < m holds epoch r's commit alone and bin m the other E - m
#                  (E > m); exact when B > N - 1: bin N - 1 = E - N + 1
#   max retries  = min(E - 1, N - 1)
CF_N, CF_POOL, CF_E = 300, 1000, 320


def closed_form_pool():
    return Epoch(np.ones(CF_POOL, np.uint64), np.ones(CF_POOL, np.uint8), np.arange(CF_POOL + 1, dtype=np.uint32))


def closed_form(n_bins):
    """(per-epoch (src, born), totals, histogram) of CF_E epochs"""
    k = np.arange(CF_E, dtype=np.int64)
    born = np.maximum(0, k - CF_N + 1)
    retries = np.minimum(k, CF_N - 1)
    hist = np.zeros(n_bins, np.int64)
    m = min(n_bins - 1, CF_N - 1)
    assert CF_E > m
    hist[:m] = 1
    hist[m] = CF_E - m
    totals = [CF_E, CF_E * (CF_N - 1), (CF_N - 1) + (CF_E - 1), min(CF_E - 1, CF_N - 1)]
    return list(zip(k, born)), retries, totals, hist


_cf_cache = {}


def closed_form_commits():
    """the oracle's commit bytes of the closed form's epochs (computed once)"""
    if "c" not in _cf_cache:
        tab = O.YcsbTable(16)
        ref, _, cur = host_closed_loop(dvcc.NO_WAIT, tab, tab.f0.copy(), closed_form_pool(), 0, CF_N, CF_E)
        assert cur == (CF_N + CF_E) % CF_POOL
        _cf_cache["c"] = [c for c, _, _ in ref]
    return _cf_cache["c"]


def test_model_equals_the_closed_form():
    commits = closed_form_commits()
    for n_bins in (512, 8):
        m = TrackModel(CF_POOL, 0, CF_N, n_bins=n_bins)
        for c in commits:
            assert int(c.sum()) == 1 and c[0] == 1
            m.epoch(c)
        want, retries, totals, hist = closed_form(n_bins)
        for k, ((src, born), (s, b)) in enumerate(zip(want, m.log)):
            assert (list(s), list(b)) == ([src], [born]), k
            assert k - born == retries[k]
        assert m.epoch_end == list(range(1, CF_E + 1))
        assert m.totals == totals
        assert (m.hist == hist).all()
    assert hist[7] == CF_E - 7  # (the saturating bin of the 8-bin histogram)
    exact = closed_form(512)[3]
    assert exact[CF_N - 1] == CF_E - CF_N + 1 and exact[:CF_N - 1].sum() == CF_N - 1 and exact[CF_N:].sum() == 0


def test_retry_summary_fields_on_the_closed_form():
    _, _, totals, hist = closed_form(512)
    sts = [SimpleNamespace(committed=1, aborted=CF_N - 1, n_txn=CF_N, write_cnt=1) for _ in range(CF_E)]
    run = 3.2  # 0.01 s per epoch
    plain = stats.summary_fields(run, sts)
    assert plain == [
        ("total_runtime", 3.2), ("tput", 320 / 3.2), ("txn_cnt", 320), ("remote_txn_cnt", 0),
        ("local_txn_cnt", 320), ("local_txn_start_cnt", 96000), ("total_txn_commit_cnt", 320),
        ("local_txn_commit_cnt", 320), ("remote_txn_commit_cnt", 0), ("total_txn_abort_cnt", 95680),
        ("unique_txn_abort_cnt", 95680), ("local_txn_abort_cnt", 95680), ("remote_txn_abort_cnt", 0),
        ("txn_run_time", sum([0.01] * 320)), ("txn_run_avg_time", sum([0.01] * 320) / 320),
        ("multi_part_txn_cnt", 0), ("single_part_txn_cnt", 320), ("txn_write_cnt", 320),
        ("record_write_cnt", 320), ("parts_touched", 320), ("avg_parts_touched", 1.0)]
    got = stats.retry_summary_fields(run, sts, totals, hist, 1)
    assert [k for k, _ in got] == [k for k, _ in plain]
    d, p = dict(got), dict(plain)
    # 299 first aborts in epoch 0, one in each of the 319 epochs after it
    assert d["unique_txn_abort_cnt"] == 618 and d["total_txn_abort_cnt"] == 95680
    # epochs charged: sum_{k < 299} (k + 1) + 21 * 300 = 44,850 + 6,300
    assert abs(d["txn_run_time"] - 51150 * 0.01) < 1e-9
    assert abs(d["txn_run_avg_time"] - 51150 * 0.01 / 320) < 1e-9
    for k in p:
        if k not in ("unique_txn_abort_cnt", "txn_run_time", "txn_run_avg_time"):
            assert d[k] == p[k], k
    # a penalty of 4 epochs (four lanes): (4 r + 1) epochs per commit
    d4 = dict(stats.retry_summary_fields(run, sts, totals, hist, 4))
    assert abs(d4["txn_run_time"] - (4 * (51150 - 320) + 320) * 0.01) < 1e-9
    line = stats.retry_summary_line(run, sts, totals, hist, 1)
    assert line.startswith("[summary] total_runtime=3.200000,") and ",unique_txn_abort_cnt=618," in line
    assert stats.summary_line(run, sts).count("unique_txn_abort_cnt=95680") == 1


def _desc(**kw):
    """a well-formed dv_loop_track over made-up addresses (never dereferenced
    by the attach call), with fields overridden"""
    ids = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    d = dict(ids=ids, n_bufs=2, first_epoch=0, log=0x3000, log_cap=100, epoch_cap=8, log_pos=0x4000,
             epoch_end=0x5000, retry_hist=0x6000, n_bins=16, totals=0x7000)
    d.update(kw)
    return L.LoopTrackDesc(d["ids"], d["n_bufs"], d["first_epoch"], d["log"], d["log_cap"], d["epoch_cap"],
                           d["log_pos"], d["epoch_end"], d["retry_hist"], d["n_bins"], d["totals"])


def malformed_descs():
    """(name, struct): each refused with DV_ERR_ARG at attach time"""
    null_ids = (ctypes.c_void_p * 2)(0x1000, None)
    return [("ids", _desc(ids=None)), ("ids entry", _desc(ids=null_ids)), ("n_bufs 0", _desc(n_bufs=0)),
            ("n_bufs odd", _desc(n_bufs=1)), ("n_bufs 18", _desc(n_bufs=18)), ("log", _desc(log=None)),
            ("log_cap", _desc(log_cap=0)), ("epoch_cap", _desc(epoch_cap=0)), ("log_pos", _desc(log_pos=None)),
            ("epoch_end", _desc(epoch_end=None)), ("retry_hist", _desc(retry_hist=None)), ("n_bins 0", _desc(n_bins=0)),
            ("n_bins 1025", _desc(n_bins=1025)), ("totals", _desc(totals=None))]


def test_track_entry_refuses_a_null_context():
    """no context, no device: DV_ERR_ARG for a detach, a well-formed struct and
    every malformed one (a real context refuses the malformed ones with the same
    code: tests/test_loop_track_gpu.py)"""
    f = L.lib().dv_closed_loop_track
    assert f(None, None) == L.DV_ERR_ARG
    assert f(None, ctypes.byref(_desc())) == L.DV_ERR_ARG
    for name, d in malformed_descs():
        assert f(None, ctypes.byref(d)) == L.DV_ERR_ARG, name


def test_loop_track_layout_matches_the_header(tmp_path):
    """the ctypes mirror of dv_loop_track against the header, compiled by gcc"""
    name, cls = "dv_loop_track", L.LoopTrackDesc
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
    assert ("dv_closed_loop_track", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(cls)]) in L.SIGNATURES
