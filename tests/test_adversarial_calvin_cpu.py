"""The closed-form CALVIN epochs of tests/adversarial_calvin.py on the CPU:
every family instance's formula against `serial_model` against the oracle --
grant groups, read digest, write count, the whole F0 column and all-commit --
and the same again for a second run on the same table, where the rows the
first run wrote now hold 0.  Then `serial_model` against the oracle on random
epochs with repeats and empty txns.

A disagreement here means the formula, the model or the oracle is wrong, and
is settled from the reference's text (txn.cpp:778-788, row_lock.cpp:78-81,
152-170, 318-358, ycsb_txn.cpp:255-353).  All three agree as committed.

Also shown by arithmetic: which sorted positions the repeat runs take, that
the hidden write's readers lie in later tiles than the write, and that the
comb's queue heads fall on every position of a thread's chunk.
"""
import functools

import numpy as np
import pytest

import _oracle as O
import adversarial_calvin as AC
from adversarial_calvin import K
from dvcc import Epoch

RD, WR = AC.RD, AC.WR


def _hold(case, runs=2):
    """formula == serial_model == oracle over `runs` runs on one table"""
    e = case.epoch
    tab = O.YcsbTable(case.rows)
    f0_or = tab.f0.copy()
    f0 = AC.initial_f0(case.rows)
    assert np.array_equal(f0, f0_or), "the F0 initialiser"
    pkey = np.arange(case.rows, dtype=np.uint64)
    for run in range(runs):
        what = f"{case.name} run {run}"
        digest, writes, f0_formula = AC.outcome(case, f0)
        g_m, digest_m, writes_m, f0_m = AC.serial_model(e, f0, pkey)
        c, g, st = O.epoch_run(O.CALVIN, tab.ix, f0_or, e.n_txn, e.txn_begin, e.keys, e.types, want_grant=True)
        assert c.all() and st.committed == e.n_txn and st.aborted == 0, what
        assert np.array_equal(case.grant, g_m), f"{what}: formula and model grants differ at {np.flatnonzero(case.grant != g_m)[:8]}"
        assert np.array_equal(g, g_m), f"{what}: oracle and model grants differ at {np.flatnonzero(g != g_m)[:8]}"
        assert digest == digest_m == st.read_digest, what
        assert writes == writes_m == st.write_cnt, what
        assert np.array_equal(f0_formula, f0_m) and np.array_equal(f0_m, f0_or), what
        f0 = f0_formula
    return f0


def test_structural_constants():
    assert K["kRTile"] == K["kBlock"] * K["kRIPT"] and K["kPV"] > 1 and K["kRIPT"] > K["kPV"]
    assert K["kRTile"] % (K["kBlock"] * K["kPV"]) == 0
    assert len(set(AC.REPEAT_B.values())) == len(AC.REPEAT_B)


# ---- repeat blocks
@pytest.mark.parametrize("what", list(AC.REPEAT_B))
def test_repeat_blocks(what):
    B = AC.REPEAT_B[what]
    cases = AC.repeat_blocks(B)
    assert len(cases) == 2 * (3 + 4 + 4)
    assert len({c.extra["hot"] for c in cases}) == len(cases)
    for case in cases:
        lo, hi = case.extra["run"]
        E = case.extra["edge"]
        assert E % B == 0 and lo - 1 <= E <= hi + 1  # the run touches the edge
        assert case.sees0.sum() == 2
        _hold(case)


def test_repeat_block_grants_by_hand():
    """first = R: P, A and Q share group 0; first = W: 0, 1, 2; Z and Q2 behind"""
    r = AC.repeat_block(4, 3, RD, "start", 1)
    w = AC.repeat_block(4, 3, WR, "start", 1)
    assert r.epoch.n_acc == w.epoch.n_acc == 3 + 1 + 3 + 3
    assert r.grant[3:].tolist() == [0, 0, 0, 0, 0, 1, 2]
    assert w.grant[3:].tolist() == [0, 1, 1, 1, 2, 3, 4]
    assert r.epoch.types[4:7].tolist() == [RD, RD, WR] and w.epoch.types[4:7].tolist() == [WR, RD, WR]
    assert np.flatnonzero(r.sees0).tolist() == np.flatnonzero(w.sees0).tolist() == [7, 9]


# ---- hidden write
@pytest.mark.parametrize("i", range(4))
def test_hidden_write(i):
    m = AC.hidden_write_sizes()[i]
    case = AC.hidden_write(m, 1 + i)
    T = K["kRTile"]
    at = case.extra["write_at"]
    last_reader = case.epoch.n_acc - 1
    if m >= T:
        assert last_reader // T > at // T, "a reader in a later tile than the write"
    if m > 3 * T:
        assert last_reader // T - at // T >= 3, "the bit travels through several tiles"
    assert not case.grant.any() and case.sees0.sum() == m
    _hold(case)


# ---- comb
@functools.lru_cache(maxsize=None)
def _combs():
    return AC.comb_epochs()


def test_comb_table_by_model():
    """every hand-written queue of the table alone against the model"""
    pkey = np.arange(2, dtype=np.uint64)
    f0 = np.array([7, 9], np.uint64)
    for txns, g, s in AC.COMB:
        types = np.array([t for txn in txns for t in txn], np.uint8)
        tb = np.r_[0, np.cumsum([len(t) for t in txns])].astype(np.uint32)
        e = Epoch(np.ones(len(types), np.uint64), types, tb)
        g_m, digest, writes, f0_after = AC.serial_model(e, f0, pkey)
        assert g_m.tolist() == g
        assert writes == int(types.sum()) and f0_after[1] == (0 if writes else 9) and f0_after[0] == 7
        case = AC.CalvinCase("q", e, 2, np.array(g, np.uint32), np.array([bool(v) for v in s]))
        assert AC.outcome(case, f0)[0] == digest


def test_comb_geometry():
    cs = _combs()
    pv, ript, T = K["kPV"], K["kRIPT"], K["kRTile"]
    assert sorted(c.epoch.n_acc % pv for c in cs[:4]) == list(range(pv))
    lo = 0
    for c in cs:  # disjoint row ranges
        used = c.epoch.keys[c.epoch.keys != 0]
        assert used.min() > lo
        lo = int(used.max())
    heads = np.concatenate([AC.head_positions(c) for c in cs])
    assert set((heads % ript).tolist()) == set(range(ript)) and set((heads % pv).tolist()) == set(range(pv))
    big = cs[4]
    h = AC.head_positions(big)
    assert big.epoch.n_acc > 3 * T
    for tile in range(3):  # a head in every thread's chunk of the first three tiles
        assert set((h[(h >= tile * T) & (h < (tile + 1) * T)] // ript % K["kBlock"]).tolist()) == set(range(K["kBlock"]))
    rev = cs[5]
    assert (np.diff(rev.epoch.keys[rev.extra["shift"]:rev.extra["shift"] + 100].astype(np.int64)) <= 0).all()


@pytest.mark.parametrize("i", range(6))
def test_comb(i):
    _hold(_combs()[i])


def test_comb_epochs_in_sequence():
    """the six epochs one after the other on one table, as the GPU tests run
    them: the formula carries F0"""
    cs = _combs()
    rows = max(c.rows for c in cs)
    tab = O.YcsbTable(rows)
    f0_or = tab.f0.copy()
    f0 = AC.initial_f0(rows)
    for c in cs:
        e = c.epoch
        digest, writes, f0 = AC.outcome(c, f0)
        _, g, st = O.epoch_run(O.CALVIN, tab.ix, f0_or, e.n_txn, e.txn_begin, e.keys, e.types, want_grant=True)
        assert np.array_equal(g, c.grant) and (st.read_digest, st.write_cnt) == (digest, writes)
        assert np.array_equal(f0, f0_or)


# ---- families 3 and 4 with their values
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_read_runs(m):
    _hold(AC.read_runs(m, 5))


@pytest.mark.parametrize("n", [1, 2, 500])
def test_writer_storm(n):
    _hold(AC.writer_storm(n))


# ---- the model against the oracle on random epochs
def _random_epoch(rng, n_txn, rows, max_len):
    lens = rng.integers(0, max_len + 1, size=n_txn)
    lens[rng.random(n_txn) < 0.1] = 0  # empty txns
    lens[0], lens[1] = 0, max_len      # (at least one empty txn and one that repeats a row)
    keys, types = [], []
    for n in lens:
        # fewer rows than accesses: every txn of two or more accesses repeats a row
        pool = rng.integers(0, rows, size=max(1, int(n) // 2))
        keys.append(pool[rng.integers(0, len(pool), size=n)])
        types.append((rng.random(n) < 0.4).astype(np.uint8))
    tb = np.r_[0, np.cumsum(lens)].astype(np.uint32)
    return Epoch(np.concatenate(keys).astype(np.uint64) if keys else np.zeros(0, np.uint64),
                 np.concatenate(types).astype(np.uint8) if types else np.zeros(0, np.uint8), tb)


@pytest.mark.parametrize("seed", range(20))
def test_serial_model_random(seed):
    rng = np.random.default_rng(1000 + seed)
    rows = int(rng.integers(3, 40))
    e = _random_epoch(rng, int(rng.integers(20, 120)), rows, int(rng.integers(2, 9)))
    tab = O.YcsbTable(rows)
    f0_or = tab.f0.copy()
    f0 = AC.initial_f0(rows)
    pkey = np.arange(rows, dtype=np.uint64)
    repeats = False
    for t in range(e.n_txn):
        k = e.keys[e.txn_begin[t]:e.txn_begin[t + 1]]
        repeats |= len(set(k.tolist())) < len(k)
    assert repeats and (np.diff(e.txn_begin.astype(np.int64)) == 0).any(), "the epoch was to hold repeats and empty txns"
    for run in range(2):
        g_m, digest, writes, f0 = AC.serial_model(e, f0, pkey)
        c, g, st = O.epoch_run(O.CALVIN, tab.ix, f0_or, e.n_txn, e.txn_begin, e.keys, e.types, want_grant=True)
        assert c.all() and st.committed == e.n_txn
        assert np.array_equal(g, g_m), f"run {run}: grants differ at {np.flatnonzero(g != g_m)[:8]}"
        assert (st.read_digest, st.write_cnt) == (digest, writes), f"run {run}"
        assert np.array_equal(f0, f0_or), f"run {run}"
