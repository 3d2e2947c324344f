"""The ragged closed-form epochs of tests/adversarial.py (family 9 and its
shapes) for the partitioned path, without a GPU.  For every shape and both
cuts -- contiguous chunks for origin-major sequences, strided chunks for
position-major ones, each origin handing over its real n_txn -- three things:

  * the oracle over dvcc.sequence / dvcc.sequence_position of the cut batches
    equals the formula under all four algorithms;
  * the cut round-trips to the global epoch array for array;
  * arithmetic from structural_constants() shows that the batches reach the
    kernel edge the shape is named for.

The last point is the evidence that test_adversarial_groups_gpu.py reaches
each edge; the kernels are not instrumented for it:

  k_group_txn_count / k_group_txn_ids / k_il_move (tiles of kXTile landed
  accesses that never span two origins, xseg_of)
      test_segment_edges: segments of kXTile - 1, kXTile, kXTile + 1 and
      2 * kXTile + 1 accesses, an origin with no access (and no txn) first,
      in the middle and last, a txn of kMaxPos accesses across a tile edge
  k_il_move_tb (tiles of kIlTxns txns, indexed through LDS up to kIlOwn
  accesses, by binary search beyond)
      test_move_tiles: tiles of at most kIlOwn accesses, exactly kIlOwn,
      kIlOwn + 1, 3 * kIlOwn with an empty txn before every run of kMaxPos-
      access txns (equal starts), and a tile of empty txns only, at
      txns_per_rank = kIlTxns - 1, kIlTxns, kIlTxns + 1 and 2 * kIlTxns + 1
  walk_committed_txns / k_route_* / k_owner_* (a wave takes 64 txns; the
  owner split)
      test_wave_mix: aligned runs of 64 slots that hold 0-, 1-, 2- and
      kMaxPos-access txns, 63 empties beside one long txn, 64 long txns; an
      owner that receives nothing and one that receives everything, at world
      3 and 8
  k_owner_* / k_ilist_bounds / k_ilist_move / k_il_begin / k_il_commits (the
  per-epoch list protocol, dv_epoch_run_part in mode 1)
      test_list_protocol_edges, test_list_protocol_wave_mix_equal_starts: home
      batches of kOwnerTile - 1, kOwnerTile, kOwnerTile + 1 and
      2 * kOwnerTile + 1 accesses and of none, owners that receive nothing or
      everything, records in a home tile past the first, and position-major
      segments that start, end and are interleaved with txns that have no
      record at the owner (equal starts under the lower bound)
"""
import functools

import numpy as np
import pytest

import adversarial as A
import dvcc
from test_adversarial_cpu import _hold

K = A.structural_constants()
X, T, OWN, M = K["kXTile"], K["kIlTxns"], K["kIlOwn"], K["kMaxPos"]
ORDERS = ("origin", "position")


def _lens(b, tpr=None):
    n = np.diff(b.txn_begin.astype(np.int64))
    return n if tpr is None else np.r_[n, np.zeros(tpr - len(n), np.int64)]


def _round_trip(case, world, order):
    """the cut of the global epoch, sequenced again: the same arrays; then
    the oracle over the sequenced batches against the formula, every
    algorithm.  Returns (batches, txns_per_rank)."""
    e = case.epoch
    parts, tpr = A.cut(e, world, order)
    assert tpr * world == e.n_txn and all(p.n_txn <= tpr for p in parts)
    seq = (dvcc.sequence_position(parts, tpr) if order == "position"
           else dvcc.sequence([A.pad_tail(p, tpr) for p in parts]))
    assert np.array_equal(seq.txn_begin, e.txn_begin)
    assert np.array_equal(seq.keys, e.keys) and np.array_equal(seq.types, e.types)
    for p in parts:  # (handed over with its real n_txn: no trailing empty txn)
        assert p.n_txn == 0 or _lens(p)[-1] > 0
    assert int(e.keys.max(initial=0)) < case.rows
    for cc in A.CCS:
        _hold(A.Case(seq, case.rows, case.expected), cc)
    return parts, tpr


def test_partitioned_constants():
    """the relations the shapes rely on; and the figure that kept the parent's
    suite out of k_il_move_tb's search branch: its batches hold 10 accesses
    per txn, 2,560 per tile of kIlTxns txns against kIlOwn = 8,192"""
    assert X == K["kBlock"] * 16 and X % K["kBlock"] == 0
    assert 10 * T <= OWN < M * T, "YCSB's 10-access txns stay in the LDS index; kMaxPos-access txns leave it"
    assert 3 * OWN <= (3 * T // 4) * M, "the search tile: three txns in four of kMaxPos accesses"
    assert T - 1 >= -(-(OWN + 1) // M) and 2 * T <= OWN, "a tile holds kIlOwn + 1 accesses in txns of 2 .. kMaxPos"
    assert K["kRouteBlocks"] % K["kBlock"] == 0 and X + M < 2 * X + 1


@pytest.mark.parametrize("cc", A.CCS)
def test_ragged_ladder_formula(cc):
    """the family itself: every slot kind, a long txn, both ends empty"""
    slots = [A.EMPTY, 0, A.ONE, M - 2, A.EMPTY, A.EMPTY, 5, 0, A.ONE, 1, A.EMPTY]
    for own in A.OWNERSHIPS:
        row_of, stride = A.ownership(own, 3)
        case = A.ragged_ladder(slots, stride, row_of)
        e = case.epoch
        assert _lens(e).tolist() == [0, 2, 1, M, 0, 0, 7, 2, 1, 3, 0]
        assert len(np.unique(e.keys)) == e.n_acc - (5 - 1), "only the ladder's links repeat a row"
        exp = case.expected_commit(cc)
        assert exp.tolist() == ([1] * 11 if cc == "CALVIN" else [1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1])
        _hold(case, cc)
    assert A.ragged_ladder([A.EMPTY] * 3, 1, lambda k: k).epoch.n_acc == 0


@pytest.mark.parametrize("world", [2, 3, 8])
def test_strided_chunks(world):
    e = A.ladder(301, empties=True).epoch
    parts, tpr = A.strided_chunks(e, world)
    assert tpr == -(-e.n_txn // world) and sum(p.n_txn for p in parts) == e.n_txn
    seq = dvcc.sequence_position(parts, tpr)
    assert np.array_equal(seq.txn_begin[:e.n_txn + 1], e.txn_begin) and (seq.txn_begin[e.n_txn:] == e.n_acc).all()
    assert np.array_equal(seq.keys, e.keys) and np.array_equal(seq.types, e.types)
    for q, p in enumerate(parts):
        assert np.array_equal(_lens(p), _lens(e)[q::world])
    t = A.trim_tail(parts[1])  # (slots 1, 1 + world, ...)
    assert t.n_txn <= parts[1].n_txn and (t.n_txn == 0 or _lens(t)[-1] > 0) and t.n_acc == parts[1].n_acc
    assert A.pad_tail(t, tpr).n_txn == tpr


@functools.lru_cache(maxsize=None)
def _segments(world, order):
    return A.segment_edge_group(world, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("world", [3, 4, 8])
def test_segment_edges(world, order):
    cases, tpr = _segments(world, order)
    assert len(cases) == world
    sizes, zero_at, straddle, tiles = set(), set(), 0, set()
    for case in cases:
        parts, tpr_ = _round_trip(case, world, order)
        assert tpr_ == tpr
        for q, p in enumerate(parts):
            sizes.add(p.n_acc)
            tiles.add(-(-p.n_acc // X))
            n = _lens(p)
            assert (n > 0).all(), "dense batches: the compact form with start bits admits them"
            if p.n_acc == 0:
                assert p.n_txn == 0  # (run_group's n_txn == 0; no tile, xseg_of skips it)
                zero_at.add(q)
            tb = p.txn_begin.astype(np.int64)
            edges = np.arange(X, p.n_acc, X)
            for edge in edges:  # a txn of kMaxPos accesses with the tile edge inside it
                j = int(np.searchsorted(tb, edge, side="right")) - 1
                straddle += int(tb[j] < edge < tb[j + 1] and n[j] == M)
        assert sum(p.n_acc == 0 for p in parts) == 1
    assert sizes == {0, X - 1, X, X + 1, 2 * X + 1}
    assert tiles == {0, 1, 2, 3}
    assert zero_at == {0, world // 2, world - 1} and len(zero_at) == 3
    assert straddle >= 1


@functools.lru_cache(maxsize=None)
def _moves(world, tpr):
    return A.move_tile_group(world, tpr)


@pytest.mark.parametrize("tpr", [T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("world", [2, 3])
def test_move_tiles(world, tpr):
    cases, tpr_ = _moves(world, tpr)
    assert tpr_ == tpr and len(cases) == world
    kinds = set()
    inner_empty_tile = short = nondense = 0
    for case in cases:
        parts, t = _round_trip(case, world, "position")
        assert t == tpr
        for p in parts:
            short += p.n_txn < tpr
            n = _lens(p, tpr)
            used = np.flatnonzero(n)
            nondense += bool(used.size and (n[:used[-1]] == 0).any())
            for j0 in range(0, tpr, T):  # k_il_move_tb's tiles of this origin
                m = n[j0:j0 + T]
                a = int(m.sum())
                if len(m) < T - 1:
                    kinds.add("small")
                    assert 0 < a <= OWN
                    continue
                if a == 0:
                    kinds.add("empties")
                    inner_empty_tile += j0 + T < p.n_txn
                elif a == OWN:
                    kinds.add("exact")
                elif a == OWN + 1:
                    kinds.add("over")  # (the first size that takes the search)
                elif a > 2 * OWN:
                    # the search, with ties: an empty txn's start equals the next txn's
                    tie = (m[:-1] == 0) & (m[1:] == M)
                    assert tie.sum() >= len(m) // 4 - 1
                    assert abs(a - 3 * OWN) <= 2 * M
                    kinds.add("search")
                else:
                    assert 0 < a < OWN
                    kinds.add("small")
    big = world * world * sum(min(T, tpr - j0) >= T - 1 for j0 in range(0, tpr, T))
    want = set(A.MOVE_KINDS[:min(big, len(A.MOVE_KINDS))]) | ({"small"} if tpr % T not in (0, T - 1) else set())
    assert kinds == want and {"search", "exact", "over", "empties"} <= kinds
    assert nondense, "an inner empty txn: compact batches need the boundaries (or go wide)"
    if tpr > T:
        assert inner_empty_tile, "a tile of empty txns with txns after it"
    else:
        assert short, "a tile of empty txns as a batch of fewer txns (down to 0)"


@functools.lru_cache(maxsize=None)
def _wave(world, own, shift=0):
    return A.wave_mix(world, own, shift)


@pytest.mark.parametrize("own", A.OWNERSHIPS)
@pytest.mark.parametrize("world", [3, 8])
def test_wave_mix(world, own):
    for shift in range(0, 3 * world, 3):  # (the epochs of the GPU file's groups)
        case = _wave(world, own, shift)
        e = case.epoch
        n = _lens(e)
        runs = [n[i:i + 64] for i in range(0, len(n) - 63, 64)]  # what one wave of the route's walk takes
        assert sum({0, 1, 2, M} <= set(r.tolist()) for r in runs) >= 4
        assert any((r == 0).sum() == 63 and r.max() == M for r in runs)
        assert any((r == M).all() for r in runs), "64 longest txns: the wave's prefix sums at their largest"
        assert e.n_txn % world == 0
        hist = np.bincount((e.keys % np.uint64(world)).astype(np.int64), minlength=world)
        if own == "spread":
            assert hist.min() > 0
        elif own == "part0":
            assert hist[0] == e.n_acc and not hist[1:].any()  # everything / nothing
        else:
            assert hist[world - 1] == 0 and hist[:world - 1].min() > 0 and hist[0] == hist.max()
        for order in ORDERS:
            parts, _ = _round_trip(case, world, order)
            inner = 0
            for p in parts:
                m = _lens(p)
                used = np.flatnonzero(m)
                inner += bool(used.size and (m[:used[-1]] == 0).any())
            assert inner, "not dense: these batches go wide, or bring their boundaries"


# ---- the list protocol (dv_epoch_run_part in mode 1), one epoch at a time:
# what test_wave_mix_part and test_segment_edges_part put in front of the
# owner split (k_owner_count / k_owner_scan / k_owner_scatter, tiles of
# kOwnerTile home accesses) and of the position-major interleave
# (k_ilist_bounds' lower bound per txn, k_ilist_move, k_il_begin, k_il_commits)
KT = K["kOwnerTile"]


def _owner_view(p, world, tpr):
    """of one origin's batch, per owner (row % world): its record count, the
    home tiles its records sit in, and which of the origin's tpr txn slots
    have a record there"""
    tb = p.txn_begin.astype(np.int64)
    own = (p.keys % np.uint64(world)).astype(np.int64)
    txn = np.repeat(np.arange(p.n_txn), np.diff(tb))
    out = []
    for o in range(world):
        at = np.flatnonzero(own == o)
        has = np.zeros(tpr, bool)
        has[txn[at]] = True
        out.append((len(at), set((at // KT).tolist()), has))
    return out


def _runs_without(has):
    """lengths of the runs of txns without a record, in order"""
    d = np.diff(np.r_[0, (~has).astype(np.int64), 0])
    return (np.flatnonzero(d == -1) - np.flatnonzero(d == 1)).tolist()


@functools.lru_cache(maxsize=None)
def _segments_own(world, order, own):
    return A.segment_edge_group(world, order, own)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("own", A.OWNERSHIPS)
@pytest.mark.parametrize("world", [3, 4])
def test_list_protocol_edges(world, own, order):
    """test_segment_edges_part's epochs, cut as it cuts them.  The owner
    split tiles the home batch by kOwnerTile == kXTile accesses, so family 9's
    segment sizes are its edges: home batches of kTile - 1, kTile, kTile + 1
    and 2 * kTile + 1 accesses (1, 1, 2 and 3 tiles) and one of 0 (no txns:
    n_home == 0).  part0: one owner receives every record, the others none
    (n_recv == 0); skip_last: the last owner receives none.  spread: every
    owner has records in a home tile b > 0 of the batches of more than a tile
    (counts[o][b], b > 0: its run of records in the send area crosses the tile
    edge), and position-major every origin that hands over fewer txns than
    txns_per_rank leaves every owner a segment whose last txns (130 of 263)
    have no record: k_ilist_bounds' lower bounds end in equal starts up to the
    segment's length."""
    assert KT == X, "the owner split's tile is the landed tile: the segment sizes are its edges too"
    cases, tpr = _segments_own(world, order, own)
    sizes, later_tile, tail_runs = set(), np.zeros(world, np.int64), np.zeros(world, np.int64)
    for case in cases:
        parts, tpr_ = _round_trip(case, world, order)
        assert tpr_ == tpr
        recv = np.zeros(world, np.int64)
        for p in parts:
            sizes.add(p.n_acc)
            assert (p.n_acc == 0) == (p.n_txn == 0)
            for o, (n, tiles, has) in enumerate(_owner_view(p, world, tpr)):
                recv[o] += n
                later_tile[o] += bool(tiles - {0})
                if n and order == "position" and p.n_txn < tpr:
                    runs = _runs_without(has)
                    assert not has[-1] and runs[-1] >= tpr - p.n_txn == 130
                    tail_runs[o] += 1
        assert sum(p.n_txn == 0 for p in parts) == 1
        if own == "part0":
            assert recv[0] == case.epoch.n_acc and not recv[1:].any()
        elif own == "skip_last":
            assert recv[-1] == 0 and recv[:-1].min() > 0
        else:
            assert recv.min() > 0
    assert sizes == {0, KT - 1, KT, KT + 1, 2 * KT + 1}
    used = world - 1 if own == "skip_last" else 1 if own == "part0" else world
    assert (later_tile[:used] >= 1).all(), "an owner's records in a home tile past the first (the 2 * kTile + 1 batch)"
    if order == "position":
        assert (tail_runs[:used] >= world).all(), "segments that end in txns without a record"


@pytest.mark.parametrize("world", [3, 8])
def test_list_protocol_wave_mix_equal_starts(world):
    """test_wave_mix_part's (1, position) run under `spread`: origin 0's first
    slot is the epoch's first, an empty txn, so every owner's segment from
    origin 0 starts with a txn without a record (tbo[0] == tbo[1] == 0); and
    since most txns hold 0, 1 or 2 accesses, every owner's segment from every
    origin has txns without a record inside it, in runs of up to 24 at world 3
    (59, 58 and 70 of origin 0's 128 txns at owners 0, 1, 2) and of up to 12
    at world 8 (31 of 48).  The batch crosses a home tile edge at world 3
    (5,822 .. 6,076 accesses an origin) and stays inside one at world 8."""
    e = _wave(world, "spread").epoch
    parts, tpr = A.cut(e, world, "position")
    for q, p in enumerate(parts):
        for o, (n, tiles, has) in enumerate(_owner_view(p, world, tpr)):
            runs = _runs_without(has)
            assert n > 0 and sum(runs) >= tpr // 3 and max(runs) >= 4
            assert has[-1], "the wave mix's last slots hold txns of kMaxPos accesses: a record at every owner"
            if q == 0:
                assert not has[0] and np.array_equal(has, has[:tpr])
            assert (tiles == {0, 1}) == (world == 3)
    v = _owner_view(parts[0], world, tpr)
    if world == 3:
        assert [int((~has).sum()) for _, _, has in v] == [59, 58, 70] and tpr == 128
        assert max(max(_runs_without(has)) for _, _, has in v) == 24
    else:
        assert int((~v[0][2]).sum()) == 31 and tpr == 48
