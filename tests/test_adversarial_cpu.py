"""The closed-form epochs of tests/adversarial.py against the CPU oracle:
commit bytes, CALVIN grant groups where a formula is stated, the counts, and
family 8's carried epoch through `host_carry`.

A disagreement here means the oracle or the formula is wrong; the ruling is
settled from the reference's text (row_lock.cpp:52-217, occ.cpp:116-239,
txn.cpp:778-788).  Every formula agrees with the oracle as committed; no
ruling was needed.

Sizes are small where the formula does not depend on size; the GPU file runs
the sizes that reach the kernels' edges.
"""
import functools

import numpy as np
import pytest

import _oracle as O
import adversarial as A
from test_carry import host_carry

OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}


def _oracle(case, cc, f0=None):
    tab = O.YcsbTable(case.rows)
    f0 = tab.f0.copy() if f0 is None else f0
    e = case.epoch
    return O.epoch_run(OCC_ID[cc], tab.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types, want_grant=cc == "CALVIN")


def _hold(case, cc, grant_formula=True):
    c, g, st = _oracle(case, cc)
    exp = case.expected_commit(cc)
    assert exp.dtype == np.uint8 and len(exp) == case.epoch.n_txn
    bad = np.flatnonzero(c != exp)
    assert bad.size == 0, f"{cc}: oracle and formula differ at txns {bad[:8]} ({bad.size} in all)"
    assert st.committed == int(exp.sum()) and st.aborted == int((1 - exp).sum())
    if cc == "CALVIN" and grant_formula and case.grant is not None:
        assert np.array_equal(g, case.grant), f"grant groups differ at {np.flatnonzero(g != case.grant)[:8]}"


@functools.lru_cache(maxsize=None)
def _consts():
    return A.structural_constants()


def test_structural_constants_parse():
    """the source's geometry, whatever the build's overrides make it: every
    constant is found, and the relations the cases rely on hold"""
    c = _consts()
    assert all(isinstance(v, int) and v > 0 for v in c.values()), c
    assert c["kTile"] % c["kAsyncThreads"] == 0 and c["kAsyncCap"] % c["kAsyncThreads"] == 0
    assert c["kTailCap64"] < c["kTailCap32"]
    assert c["kHotRows"] & (c["kHotRows"] - 1) == 0 and c["kBloomBits"] & (c["kBloomBits"] - 1) == 0


@pytest.mark.parametrize("cc", A.CCS)
@pytest.mark.parametrize("L", [1, 2, 7, 300])
def test_ladder(cc, L):
    _hold(A.ladder(L), cc)


@pytest.mark.parametrize("cc", A.CCS)
@pytest.mark.parametrize("L,f", [(1, 0), (6, 0), (7, 3), (301, 5)])
def test_ladder_hot(cc, L, f):
    case = A.ladder_hot(L, f)
    if f == 5:
        assert case.extra["hot_share"] >= 0.6
    _hold(case, cc)


@pytest.mark.parametrize("cc", A.CCS)
@pytest.mark.parametrize("L,n", [(1, 3), (2, 3), (300, 1200), (301, 1200)])
def test_ladder_gate(cc, L, n):
    """both outcomes of the gate: L odd, it commits and the readers abort;
    L even, it aborts and they commit"""
    case = A.ladder_gate(L, n)
    if cc != "CALVIN":
        assert case.expected_commit(cc)[L:].all() == (L % 2 == 0)
    if L >= 300:
        assert case.extra["hot_share"] >= 0.6
    _hold(case, cc)


@pytest.mark.parametrize("cc", A.CCS)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_read_runs(cc, m):
    _hold(A.read_runs(m, 5), cc)


@pytest.mark.parametrize("cc", A.CCS)
@pytest.mark.parametrize("n", [1, 2, 500])
def test_writer_storm(cc, n):
    _hold(A.writer_storm(n), cc)


@pytest.mark.parametrize("cc", A.CCS)
@pytest.mark.parametrize("x", [A.RD, A.WR])
def test_self_conflict(cc, x):
    _hold(A.self_conflict(x), cc)


@pytest.mark.parametrize("cc", ["NO_WAIT", "WAIT_DIE", "OCC"])
@pytest.mark.parametrize("sweep_wr", [0, 1])
@pytest.mark.parametrize("acc_mod", [1, 63])
def test_row_sweep(cc, sweep_wr, acc_mod):
    """a small table with the same shape: the hot-row boundary inside it and a
    partial last bitmap word (rows % 16 = 5)"""
    rows = 2 * _consts()["kHotRows"] + 37
    case = A.row_sweep(rows, 512, sweep_wr, acc_mod)
    assert case.extra["prefix_acc"] % 64 == acc_mod
    e = case.epoch
    assert e.n_txn == 512 + (rows + 15) // 16
    k = e.keys[:case.extra["prefix_acc"]]
    assert {_consts()["kHotRows"] - 1, _consts()["kHotRows"], rows - 1, rows - 38} <= set(k.tolist())
    exp = case.expected_commit(cc)
    assert exp[:512].all() and 0 < int((exp[512:] == 0).sum()) < 1024 * (2 if sweep_wr else 1)
    _hold(case, cc)


@pytest.mark.parametrize("cc", ["NO_WAIT", "OCC"])
def test_width_boundary_shape(cc):
    """the family at a small size (its own sizes, 2^22 and 2^22 + 1, run on
    the GPU against the oracle and the formula)"""
    case = A.width_boundary(5000, L=301)
    e = case.epoch
    assert e.n_txn == 5000 and e.max_txn_acc() == 128
    assert int(e.txn_begin[5000 - 301]) - int(e.txn_begin[5000 - 302]) == 128
    _hold(case, cc)


@pytest.mark.parametrize("cc", ["NO_WAIT", "WAIT_DIE", "OCC"])
@pytest.mark.parametrize("which", ["ladder", "blocks"])
def test_carried_epochs(cc, which):
    """family 8: the closed-form commit bytes, the carried epoch `host_carry`
    forms from them (whole and capped one below the carried count), and the
    carried epoch run next: all of it commits"""
    case = A.ladder(301, empties=True) if which == "ladder" else A.carry_blocks(256)
    _hold(case, cc)
    e, exp, want = case.epoch, case.expected_commit(cc), case.carried
    if which == "ladder":
        assert want.n_txn == 301 // 2 and want.n_acc == 2 * (301 // 2)
    else:
        assert want.n_txn == 256 + 19
        for blk, kind in enumerate((1, 1, 0, 1)):  # whole blocks: empty, commit, abort, commit
            assert (exp[256 * blk:256 * (blk + 1)] == kind).all()
        assert (np.diff(e.txn_begin.astype(np.int64))[:256] == 0).all()
    for cap in (e.n_txn, want.n_txn - 1):
        hc = host_carry(e, exp, cap)
        n = min(cap, want.n_txn)
        assert hc.n_txn == n
        assert np.array_equal(hc.txn_begin, want.txn_begin[:n + 1])
        assert np.array_equal(hc.keys, want.keys[:hc.n_acc]) and np.array_equal(hc.types, want.types[:hc.n_acc])
    # the next epoch, on the table the first one left
    tab = O.YcsbTable(case.rows)
    f0 = tab.f0.copy()
    O.epoch_run(OCC_ID[cc], tab.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types)
    c2, _, st2 = O.epoch_run(OCC_ID[cc], tab.ix, f0, want.n_txn, want.txn_begin, want.keys, want.types)
    assert c2.all() and st2.committed == want.n_txn and st2.aborted == 0


def test_contiguous_chunks():
    e = A.ladder(301).epoch
    for world in (2, 8):
        parts, tpr = A.contiguous_chunks(e, world)
        assert tpr == -(-301 // world) and sum(p.n_txn for p in parts) == 301
        assert np.array_equal(np.concatenate([p.keys for p in parts]), e.keys)
        assert all(p.n_txn == tpr for p in parts[:-1]) and int(parts[0].txn_begin[-1]) == 2 * tpr
