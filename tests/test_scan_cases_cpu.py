"""DV_SCAN accesses on the CPU: the substituted closed-form epochs of
tests/scan_cases.py against the oracle under all four algorithms -- commit
bytes, CALVIN's grant groups, the write count, the whole F0 column and the
read digest, every one against the formulas (scan_cases.reference) -- against
the multi-threaded CPU baseline (oracle/mt_engine.c) on one thread, and
through the host-side record builders.

A disagreement is settled from the reference's text: a SCAN takes LOCK_SH
(storage/row.cpp:191, :228) and reads the row (row.cpp:257,
benchmarks/ycsb_txn.cpp:228).  The oracle as it stood left a SCAN's read out of
CALVIN's read digest (its execution loop added `types[a] == OR_RD` alone);
test_calvin_batches and test_oracle[...-CALVIN-...] failed on it, and it now
counts RD and SCAN as the reference does.  The locking and OCC loops already
counted every access that is no write.

tests/golden/ holds no SCAN (test_golden_epochs_hold_no_scan), so no fixture
moved.
"""
import os

import numpy as np
import pytest

import _oracle as O
import adversarial as A
import adversarial_calvin as AC
import loop_cases as LC
import scan_cases as S
import dvcc
from dvcc import Epoch
from test_loop_track import TrackModel

OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}
CASES = [(name, cc) for name, (_, ccs) in S.FAMILIES.items() for cc in ccs]


def _oracle(cc, tab, f0, e):
    return O.epoch_run(OCC_ID[cc], tab.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types, want_grant=cc == "CALVIN")


# ---- the helper itself
@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_substitution_is_by_position(name, pattern):
    """only reads change, to 3, exactly at the pattern's positions; keys and
    boundaries stay; what the case expects is the same object as before"""
    base = S.pad_reads(S.family(name), 1 + list(S.FAMILIES).index(name) % 3) if pattern == "edge" else S.family(name)
    sub = S.scan_substitute(base, pattern)
    e0, e1 = base.epoch, sub.epoch
    assert np.array_equal(e0.keys, e1.keys) and np.array_equal(e0.txn_begin, e1.txn_begin)
    changed = e0.types != e1.types
    assert changed.any() and (e0.types[changed] == A.RD).all() and (e1.types[changed] == S.SCAN).all()
    a = np.arange(e0.n_acc)
    where = {"all": np.ones(e0.n_acc, bool), "mod3": a % 3 == 0, "edge": a >= e0.n_acc - e0.n_acc % 4}[pattern]
    assert np.array_equal(changed, where & (e0.types == A.RD))
    assert sub.expected is base.expected and sub.grant is base.grant and sub.extra is base.extra
    if pattern == "mod3" and name in ("carry_ladder", "carry_blocks", "sweep_63"):
        # a packed word of four type bytes mixes all three values
        w = e1.types[:e1.n_acc // 4 * 4].reshape(-1, 4)
        assert any({0, 1, 3} <= set(r.tolist()) for r in w)
    if pattern == "edge":
        assert e1.n_acc % 4 and (e1.types[-(e1.n_acc % 4):] == S.SCAN).all() and not changed[:-(e1.n_acc % 4)].any()
    if base.carried is not None:
        idx = S._gather(e1.txn_begin, base.extra["carried_from"])
        assert np.array_equal(sub.carried.types, e1.types[idx]) and np.array_equal(sub.carried.keys, base.carried.keys)
        assert (base.expected["NO_WAIT"][base.extra["carried_from"]] == 0).all()
        assert int((base.expected["NO_WAIT"] == 0).sum()) == base.carried.n_txn


def test_read_digest_closed_form_by_hand():
    """two txns on a 3-row table, NO_WAIT: [R 0, SCAN 1] commits, [W 1] meets
    the shared lock and aborts; the digest is the two terms of dvcc.h's
    formula, written out"""
    def m(z):  # splitmix64's finalizer (dvcc.h's mix64), in Python integers
        z &= M
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M
        return z ^ (z >> 31)
    M = (1 << 64) - 1
    e = Epoch(np.uint64([0, 1, 1]), np.uint8([0, 3, 1]), np.uint32([0, 2, 3]))
    case = A.Case(e, 3, {"NO_WAIT": np.uint8([1, 0])})
    f0 = AC.initial_f0(3)
    ref = S.reference(case, "NO_WAIT", f0)
    want = (m(int(f0[0]) ^ m((0 << 32) ^ 0)) + m(int(f0[1]) ^ m((0 << 32) ^ 1))) % (1 << 64)
    assert ref.digest == want and ref.writes == 0 and np.array_equal(ref.f0, f0)


# ---- the oracle, all four algorithms
@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("name,cc", CASES)
def test_oracle(name, cc, pattern):
    case = S.substituted(name, pattern)
    e = case.epoch
    tab = O.YcsbTable(case.rows)
    f0 = tab.f0.copy()
    assert np.array_equal(f0, AC.initial_f0(case.rows)), "the F0 initialiser"
    ref = S.reference(case, cc, f0)
    c, g, st = _oracle(cc, tab, f0, e)
    S.held(ref, c, g, st, f0, f"{name} {pattern} {cc}")
    if case.carried is not None and cc != "CALVIN":
        # the carried epoch next, on the table the first left: all of it commits
        nxt = A.Case(case.carried, case.rows, {cc: np.ones(case.carried.n_txn, np.uint8)})
        ref2 = S.reference(nxt, cc, ref.f0)
        c2, _, st2 = _oracle(cc, tab, f0, nxt.epoch)
        S.held(ref2, c2, None, st2, f0, f"{name} {pattern} {cc}: the carried epoch")


@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("batch", list(S.CALVIN_BATCHES))
def test_calvin_batches(batch, pattern):
    """CALVIN's own families, a batch's epochs one after the other on one
    table, twice over: in a shared group a SCAN opens no new grant group, next
    to a write it does, and its value enters the digest"""
    cases, rows = S.calvin_batch(batch, pattern)
    refs = S.batch_references(cases, rows, calls=2)
    tab = O.YcsbTable(rows)
    f0 = tab.f0.copy()
    pkey = np.arange(rows, dtype=np.uint64)
    for i, ref in enumerate(refs):
        case = cases[i % len(cases)]
        e = case.epoch
        if i < len(cases):  # the formula against the serial model too
            g_m, digest_m, writes_m, f0_m = AC.serial_model(e, f0, pkey)
            assert np.array_equal(g_m, ref.grant) and (digest_m, writes_m) == (ref.digest, ref.writes), case.name
            assert np.array_equal(f0_m, ref.f0), case.name
        c, g, st = _oracle("CALVIN", tab, f0, e)
        S.held(ref, c, g, st, f0, f"{case.name} {pattern} run {i // len(cases)}")


def test_scan_beside_a_write_by_hand():
    """one row: [SCAN] [SCAN] [W] [SCAN] [RD] [W] -- the first two share group
    0, the write takes 1, the two readers behind it share 2, the write 3"""
    e = Epoch(np.full(6, 1, np.uint64), np.uint8([3, 3, 1, 3, 0, 1]), np.arange(7, dtype=np.uint32))
    case = AC.CalvinCase("by_hand", e, 2, np.uint32([0, 0, 1, 2, 2, 3]), np.array([0, 0, 0, 1, 1, 0], bool))
    tab = O.YcsbTable(2)
    f0 = tab.f0.copy()
    ref = S.reference(case, "CALVIN", f0)
    assert ref.writes == 2 and ref.f0[1] == 0 and ref.f0[0] == f0[0]
    c, g, st = _oracle("CALVIN", tab, f0, e)
    S.held(ref, c, g, st, f0, "by hand")


# ---- the CPU baseline (oracle/mt_engine.c), one thread
MT = ["runs_64", "gate_odd", "ladder_hot", "storm", "self_R", "carry_ladder"]


@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("name", MT)
def test_mt_engine_one_thread(name, pattern):
    """On one thread the baseline runs the txns one after the other, each
    releasing its locks at its end: every txn of these families commits (none
    repeats a row it writes) and reads what the txns before it left --
    adversarial_calvin's serial model.  A SCAN takes the shared lock and its
    value enters the digest; taken for a write it would store 0 instead."""
    case = S.substituted(name, pattern)
    e = case.epoch
    tab = O.YcsbTable(case.rows)
    f0 = tab.f0.copy()
    _, digest, writes, f0_after = AC.serial_model(e, f0, np.arange(case.rows, dtype=np.uint64))
    assert writes == int((e.types == A.WR).sum())
    lock = O.mt_lock(case.rows)
    committed, got = O.mt_epoch_run(tab.ix, f0, lock, e.n_txn, e.txn_begin, e.keys, e.types, 1)
    assert committed == e.n_txn
    assert got == digest, f"read digest {got:#x}, serial model {digest:#x}"
    assert np.array_equal(f0, f0_after) and not lock.any()


# ---- the closed loop's pool
@pytest.mark.parametrize("pattern", ["all", "mod3"])
@pytest.mark.parametrize("cc", S.DECIDING)
def test_closed_loop_model(cc, pattern):
    """loop_cases' hot-row pool with SCANs through the host model of the closed
    loop (carried txns first, then fresh ones): every epoch's oracle outcome
    against the commit formula and the closed-form digest, and the refilled
    epochs hold the byte 3 where their pool txns do"""
    p = S.loop_pool(pattern)
    model = TrackModel(p.P, 0, S.LOOP_N)
    ref, left, f0_or = LC.run_model(getattr(dvcc, cc), p, model, S.LOOP_EPOCHS)
    f0 = AC.initial_f0(p.rows)
    for k, (c, st, host) in enumerate(ref):
        r, h = S.loop_epoch_reference(p, cc, model.seen[k][0], f0)
        assert np.array_equal(h.types, host.types) and (host.types == S.SCAN).any()
        S.held(r, c, None, st, None, f"epoch {k}")
        f0 = r.f0
    assert np.array_equal(f0, f0_or)
    nxt = left[S.LOOP_EPOCHS]
    carried = int((ref[-1][0] == 0).sum())
    assert carried > 0 and (nxt.types[:int(nxt.txn_begin[carried])] == S.SCAN).any()


# ---- the host-side record builders
@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("name", ["gate_odd", "storm", "sweep_63", "carry_blocks"])
def test_host_records(name, pattern):
    """Epoch.to_row_records (the 4-byte records of dv_epoch_stage_host_rows and
    dv_epoch_dev.recs32): a SCAN's write bit is clear, a write's set, the key
    below it; Epoch.to_access_array (dv_access of dv_epoch_run) keeps the byte"""
    e = S.substituted(name, pattern).epoch
    r = e.to_row_records()
    assert r.dtype == np.uint32 and np.array_equal(r >> 31, (e.types == A.WR).astype(np.uint32))
    assert not (r[e.types == S.SCAN] >> 31).any() and np.array_equal(r & 0x7FFFFFFF, e.keys.astype(np.uint32))
    acc = e.to_access_array()
    assert np.array_equal(acc["type"], e.types) and (acc["type"] == S.SCAN).any()
    assert np.array_equal(acc["txn_seq"], e.acc_txn()) and np.array_equal(acc["key"], e.keys)


def test_golden_epochs_hold_no_scan():
    """so the oracle's digest of every golden epoch is what it was"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    names = [f for f in os.listdir(golden) if f.endswith(".npz")]
    assert names
    for f in names:
        with np.load(os.path.join(golden, f)) as z:
            assert np.isin(z["types"], (A.RD, A.WR)).all(), f
