"""The ragged closed-form epochs (tests/adversarial.py, family 9) on the
partitioned HIP path: P engine contexts on one GPU over the in-process
transport, as test_partitioned.py runs them.  Every comparison is exact:

  * each rank's commit bytes equal the formula (computed in numpy) and the
    oracle's;
  * committed count, read digest and write count, summed over the ranks,
    equal the oracle run over the epochs one after the other;
  * every partition's rows equal the oracle's afterwards.

test_adversarial_groups_cpu.py shows by arithmetic which kernel edge each
shape reaches (segments of kXTile +- 1 accesses and origins without any,
k_il_move_tb's tiles on either side of kIlOwn and its binary search over equal
starts, waves of 0-, 1-, 2- and kMaxPos-access txns, owners that receive
nothing or everything).  Here every shape runs through every batch form it
can take:

  start_bits  compact 4-byte batches numbered again from start bits (dense
              batches, prefix kill off)
  tbx         compact batches whose txn boundaries travel beside them
              (dv_set_prefix on every decider; not CALVIN)
  wide        8-byte batches by DV_COMM_WIDE_BATCHES
  nondense    8-byte batches because a batch has an inner empty txn

origin-major (contiguous cut) and position-major (strided cut; not CALVIN,
which keeps the sequencer's order).  One engine group serves all forms and
orders of a test, the oracle's table running along.

The per-epoch list protocol (dv_epoch_run_part in mode 1: the owner split,
and position-major k_ilist_bounds / k_ilist_move / k_il_begin / k_il_commits)
takes the wave mix and the segment edges one epoch at a time, in both orders
(test_wave_mix_part, test_segment_edges_part).
"""
import functools

import numpy as np
import pytest
import torch

import _oracle as O
import adversarial as A
import dvcc
from dvcc import DeviceEpoch
from test_partitioned import _group_mine, _origin_order, _run_group, _run_group_batches, _run_group_epochs

pytestmark = pytest.mark.gpu

CC = {"NO_WAIT": dvcc.NO_WAIT, "WAIT_DIE": dvcc.WAIT_DIE, "OCC": dvcc.OCC, "CALVIN": dvcc.CALVIN}
OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}
K = A.structural_constants()
T = K["kIlTxns"]
WIDE, POSITION = dvcc._lib.DV_COMM_WIDE_BATCHES, dvcc._lib.DV_COMM_POSITION_ORDER


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield
    for f in (_segments, _moves, _waves, _segments_own):
        f.cache_clear()


def _engines(cc, world, rows_pp, tpr, caps, mode, asynchronous=False):
    """`world` contexts on one GPU, context p owning rows p, p + world, ...;
    caps[p]: its capacity in accesses, sized from the case"""
    engines = []
    for p in range(world):
        eng = dvcc.CCEngine(CC[cc], tpr * world, max(64, caps[p]), part_cnt=world, part_id=p,
                            asynchronous=asynchronous)
        eng.load_ycsb_partition(rows_pp)
        engines.append(eng)
    dvcc.CCEngine.comm_init_local(engines)
    for eng in engines:
        eng.comm_set_mode(mode)
    return engines


def _orders(cc):
    return ("origin",) if cc == "CALVIN" else ("origin", "position")


class _Table:
    """the oracle's one-partition table (row == key), running along"""

    def __init__(self, rows_pp, world):
        self.tab = O.YcsbTable(rows_pp * world)
        self.f0 = self.tab.f0.copy()
        self.world, self.rows_pp = world, rows_pp

    def run(self, cc, case):
        """the epoch on the oracle: its commit bytes -- the formula's -- and stats"""
        e = case.epoch
        c, _, st = O.epoch_run(OCC_ID[cc], self.tab.ix, self.f0, e.n_txn, e.txn_begin, e.keys, e.types)
        assert np.array_equal(c, case.expected_commit(cc)), "oracle off the formula"
        return c, st

    def check_rows(self, engines, what):
        for p, eng in enumerate(engines):
            assert np.array_equal(eng.read_table(0, self.rows_pp), self.f0[p::self.world]), f"{what}: partition {p} rows"


def _homes(cases, world, order, form):
    """[rank][epoch] device batches of a group's epochs, cut for `order`"""
    parts = [A.cut(case.epoch, world, order)[0] for case in cases]
    homes = [[DeviceEpoch(parts[e][r]) for e in range(world)] for r in range(world)]
    flat = [h for hs in homes for h in hs]
    if form == "start_bits":
        assert all(h.dense for h in flat)
    elif form == "nondense":
        assert any(h.dense is False for h in flat)
    elif form == "tbx":
        for r in range(world):
            for e in range(world):
                h = homes[r][e]
                # (density unknown, as for raw device buffers: with the
                # boundaries travelling nothing is numbered again)
                h.dense = None
                if h.n_txn == 0 and r % 2:  # a batch without txns: one boundary word, or (odd ranks) none at all
                    homes[r][e] = DeviceEpoch.from_tensors(h.keys, h.types, h.acc_txn, 0)
    return homes


def _set_form(engines, form, order, n_txn):
    for eng in engines:
        eng.set_prefix(max(2, n_txn // 4) if form == "tbx" else None)
        eng.comm_set_mode(2 | (WIDE if form == "wide" else 0) | (POSITION if order == "position" else 0))


def _check_group_result(cc, world, tpr, order, res_of, refs, cases, what, form=None):
    """res_of(r) -> (commit bytes, stats) of rank r for this group"""
    committed = sum(st.committed for _, st in refs)
    digest = writes = 0
    for r in range(world):
        c, st = res_of(r)
        for e in range(world):
            exp = cases[e].expected_commit(cc)
            mine = _group_mine(exp, r, tpr, world, CC[cc], order == "position")
            got = c[e * tpr:(e + 1) * tpr]
            assert np.array_equal(got, mine), f"{what}: epoch {e} rank {r}: {int((got != mine).sum())} txns off the formula"
            assert np.array_equal(got, _group_mine(refs[e][0], r, tpr, world, CC[cc], order == "position"))
        assert st.committed == committed == sum(int(case.expected_commit(cc).sum()) for case in cases), what
        assert st.n_txn == tpr * world * world
        if form == "tbx":
            assert st.prefix_txn, f"{what}: the decider did not take the prefix-kill path"
        digest = (digest + st.read_digest) % (1 << 64)
        writes += st.write_cnt
    assert digest == sum(st.read_digest for _, st in refs) % (1 << 64), f"{what}: read digest"
    assert writes == sum(st.write_cnt for _, st in refs), f"{what}: write count"


def _run_forms(cc, world, group_of, forms, orders=None):
    """group_of(order) -> (cases, tpr): one engine group, then every order and
    form in turn"""
    built = {order: group_of(order) for order in (orders or _orders(cc))}
    tpr = max(t for _, t in built.values())
    rows_pp = -(-max(case.rows for cases, _ in built.values() for case in cases) // world)
    # a decider receives one epoch, sends its batches of every epoch, and as an
    # owner receives at most every committed access of the group (2 x capacity)
    cap = max(sum(case.epoch.n_acc for case in cases) for cases, _ in built.values()) + 4096
    engines = _engines(cc, world, rows_pp, tpr, [cap] * world, 2)
    table = _Table(rows_pp, world)
    try:
        for order, (cases, tpr_) in built.items():
            assert tpr_ == tpr
            for form in forms:
                if form == "tbx" and cc == "CALVIN":
                    continue
                what = f"{form} {order}-major"
                _set_form(engines, form, order, tpr * world)
                homes = _homes(cases, world, order, form)
                refs = [table.run(cc, case) for case in cases]
                res = _run_group_epochs(engines, homes, tpr)
                for r, x in enumerate(res):
                    assert not isinstance(x, Exception), f"{what}: rank {r}: {x}"
                _check_group_result(cc, world, tpr, order, lambda r: res[r], refs, cases, what, form)
                table.check_rows(engines, what)
    finally:
        for eng in engines:
            eng.close()


# ---- segment edges: k_group_txn_count, k_group_txn_ids, k_il_move, xseg_of
@functools.lru_cache(maxsize=None)
def _segments(world, order):
    return A.segment_edge_group(world, order)


@pytest.mark.parametrize("cc,order", [(cc, order) for cc in A.CCS for order in _orders(cc)])
@pytest.mark.parametrize("world", [3, 4, 8])
def test_segment_edges(cc, order, world):
    """Per-origin segments of kXTile - 1, kXTile, kXTile + 1 and 2 * kXTile +
    1 accesses, an origin without accesses or txns first, in the middle and
    last, a kMaxPos-access txn across a tile edge (one group)."""
    _run_forms(cc, world, lambda o: _segments(world, o), ("start_bits", "tbx", "wide"), orders=(order,))


# ---- move tiles: k_il_move_tb (and k_il_bounds / k_il_move<WIDE> over the same batches)
@functools.lru_cache(maxsize=None)
def _moves(world, tpr, first=0):
    return A.move_tile_group(world, tpr, first=first)


@pytest.mark.parametrize("cc", ["NO_WAIT", "WAIT_DIE", "OCC"])
@pytest.mark.parametrize("tpr", [T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("world", [2, 3])
def test_move_tiles(cc, world, tpr):
    """Position-major batches that bring their boundaries, whose tiles of
    kIlTxns txns hold at most kIlOwn accesses, exactly kIlOwn, kIlOwn + 1,
    3 * kIlOwn behind runs of equal starts (the binary search) and none; then
    the same batches through both 8-byte forms (k_il_bounds, k_il_move)."""
    _run_forms(cc, world, lambda order: _moves(world, tpr), ("tbx", "wide", "nondense"), orders=("position",))


def test_move_tiles_two_groups():
    """Two groups of the move-tile shape in one dv_epoch_group_run_batch call
    (the second group's tiles take the kinds in another turn)."""
    cc, world, tpr, order = "NO_WAIT", 2, T + 1, "position"
    groups = [_moves(world, tpr)[0], _moves(world, tpr, 2)[0]]
    rows_pp = -(-max(case.rows for cases in groups for case in cases) // world)
    cap = max(sum(case.epoch.n_acc for case in cases) for cases in groups) + 4096
    engines = _engines(cc, world, rows_pp, tpr, [cap] * world, 2)
    table = _Table(rows_pp, world)
    try:
        _set_form(engines, "tbx", order, tpr * world)
        per_group = [_homes(cases, world, order, "tbx") for cases in groups]
        refs = [[table.run(cc, case) for case in cases] for cases in groups]
        res = _run_group_batches(engines, [[per_group[g][r] for g in range(2)] for r in range(world)], tpr, 2)
        for r, x in enumerate(res):
            assert not isinstance(x, Exception), f"rank {r}: {x}"
        for g, cases in enumerate(groups):
            _check_group_result(cc, world, tpr, order, lambda r: (res[r][0][g], res[r][1][g]), refs[g], cases,
                                f"group {g}", "tbx")
        table.check_rows(engines, "after both groups")
    finally:
        for eng in engines:
            eng.close()


@pytest.mark.parametrize("order", ["origin", "position"])
def test_boundaries_with_mixed_record_forms(order):
    """One rank's batches come without 4-byte records (it packs them) while
    its peers send theirs straight from their buffers: each sender picks its
    form, and the transport has to pair them -- the same results."""
    cc, world, tpr = "NO_WAIT", 2, T - 1
    cases, _ = A.move_tile_group(world, tpr, order=order)
    rows_pp = -(-max(case.rows for case in cases) // world)
    engines = _engines(cc, world, rows_pp, tpr, [sum(case.epoch.n_acc for case in cases) + 4096] * world, 2)
    table = _Table(rows_pp, world)
    try:
        _set_form(engines, "tbx", order, tpr * world)
        homes = _homes(cases, world, order, "tbx")
        parts = [A.cut(case.epoch, world, order)[0] for case in cases]
        homes[1] = [DeviceEpoch(parts[e][1], recs32=False) for e in range(world)]
        for h in homes[1]:
            h.dense = None
        assert all(h.recs32 is None for h in homes[1]) and all(h.recs32 is not None for h in homes[0])
        refs = [table.run(cc, case) for case in cases]
        res = _run_group_epochs(engines, homes, tpr)
        for r, x in enumerate(res):
            assert not isinstance(x, Exception), f"rank {r}: {x}"
        _check_group_result(cc, world, tpr, order, lambda r: res[r], refs, cases, f"{order}-major", "tbx")
        table.check_rows(engines, f"{order}-major")
    finally:
        for eng in engines:
            eng.close()


# ---- wave mix: walk_committed_txns, k_route_count / scan / scatter, the owner split
@functools.lru_cache(maxsize=None)
def _waves(world, own):
    return [A.wave_mix(world, own, shift=3 * e) for e in range(world)]


@pytest.mark.parametrize("cc,order", [(cc, order) for cc in A.CCS for order in _orders(cc)])
@pytest.mark.parametrize("own", A.OWNERSHIPS)
@pytest.mark.parametrize("world", [3, 8])
def test_wave_mix_groups(cc, order, world, own):
    """Runs of 64 slots mixing 0-, 1-, 2- and kMaxPos-access txns through the
    route's txn walk, at world 3 (not a power of two) and 8, with the rows
    spread, all on partition 0, and never on the last partition."""
    def group_of(o):
        cases = _waves(world, own)
        return cases, cases[0].epoch.n_txn // world
    _run_forms(cc, world, group_of, ("tbx", "wide", "nondense"), orders=(order,))


@pytest.mark.parametrize("cc", A.CCS)
@pytest.mark.parametrize("own", A.OWNERSHIPS)
@pytest.mark.parametrize("world", [3, 8])
def test_wave_mix_part(cc, world, own):
    """The per-epoch protocols over the wave mix: the list protocol (mode 1:
    k_owner_count / scan / scatter see an owner that receives nothing and one
    that receives everything) in both orders -- position-major it interleaves
    the received records itself, k_ilist_bounds / k_ilist_move, over segments
    that start with txns without a record at the owner -- the replicated one
    (mode 2) and its position-major form."""
    case = A.wave_mix(world, own)
    e = case.epoch
    tpr = e.n_txn // world
    rows_pp = -(-case.rows // world)
    # (with the position flag CALVIN keeps origin order, _orders)
    modes = [(mode, order) for mode in (1, 2) for order in _orders(cc)]
    for mode, order in modes:
        parts, tpr_ = A.cut(e, world, order)
        assert tpr_ == tpr
        # the list protocol: an owner may receive every record; a replicated
        # epoch: the whole epoch, all-gathered in slots of the longest batch
        cap = max(e.n_acc, world * max(p.n_acc for p in parts)) + 4096
        engines = _engines(cc, world, rows_pp, tpr, [cap] * world, mode | (POSITION if order == "position" else 0),
                           asynchronous=mode == 1)
        what = f"mode {mode} {order}-major"
        try:
            # (a fresh group of engines: its rows start where the oracle's did)
            fresh = _Table(rows_pp, world)
            c_ref, st_ref = fresh.run(cc, case)
            exp = case.expected_commit(cc)
            if order == "position":
                exp, c_ref = _origin_order(exp, world, tpr), _origin_order(c_ref, world, tpr)
            res = _run_group(engines, [DeviceEpoch(p) for p in parts], tpr)
            digest = writes = 0
            for r, x in enumerate(res):
                assert not isinstance(x, Exception), f"{what}: rank {r}: {x}"
                c, st = x
                assert np.array_equal(c, exp), f"{what}: rank {r}: {int((c != exp).sum())} txns off the formula"
                assert np.array_equal(c, c_ref)
                assert st.committed == st_ref.committed == int(exp.sum())
                digest = (digest + st.read_digest) % (1 << 64)
                writes += st.write_cnt
            assert digest == st_ref.read_digest and writes == st_ref.write_cnt, what
            fresh.check_rows(engines, what)
        finally:
            for eng in engines:
                eng.close()


# ---- segment edges through the list protocol: the owner split's tiles, k_ilist_bounds / k_ilist_move
@functools.lru_cache(maxsize=None)
def _segments_own(world, order, own):
    return A.segment_edge_group(world, order, own)


@pytest.mark.parametrize("cc,order", [(cc, order) for cc in A.CCS for order in _orders(cc)])
@pytest.mark.parametrize("own", A.OWNERSHIPS)
@pytest.mark.parametrize("world", [3, 4])
def test_segment_edges_part(cc, order, world, own):
    """The segment-edge epochs one at a time through the list protocol (mode
    1), one dv_epoch_run_part call each on one engine group, the oracle's
    table running along: home batches of kTile - 1, kTile, kTile + 1 and
    2 * kTile + 1 accesses in front of k_owner_count / scan / scatter, an
    origin without txns (n_home == 0), and with the rows all on partition 0 or
    never on the last one owners that receive nothing (n_recv == 0).  Every
    batch is handed over with its real n_txn: position-major the shorter
    segments end in txns without a record (test_adversarial_groups_cpu.py,
    test_list_protocol_edges)."""
    cases, tpr = _segments_own(world, order, own)
    rows_pp = -(-max(case.rows for case in cases) // world)
    cap = max(case.epoch.n_acc for case in cases) + 4096  # (an owner may receive every record)
    engines = _engines(cc, world, rows_pp, tpr, [cap] * world, 1 | (POSITION if order == "position" else 0),
                       asynchronous=True)
    table = _Table(rows_pp, world)
    try:
        for k, case in enumerate(cases):
            what = f"epoch {k} {order}-major"
            parts, tpr_ = A.cut(case.epoch, world, order)
            assert tpr_ == tpr and min(p.n_txn for p in parts) == 0
            c_ref, st_ref = table.run(cc, case)
            exp = case.expected_commit(cc)
            if order == "position":
                exp, c_ref = _origin_order(exp, world, tpr), _origin_order(c_ref, world, tpr)
            res = _run_group(engines, [DeviceEpoch(p) for p in parts], tpr)
            digest = writes = 0
            for r, x in enumerate(res):
                assert not isinstance(x, Exception), f"{what}: rank {r}: {x}"
                c, st = x
                assert np.array_equal(c, exp), f"{what}: rank {r}: {int((c != exp).sum())} txns off the formula"
                assert np.array_equal(c, c_ref)
                assert st.committed == st_ref.committed == int(exp.sum())
                digest = (digest + st.read_digest) % (1 << 64)
                writes += st.write_cnt
            assert digest == st_ref.read_digest and writes == st_ref.write_cnt, what
            table.check_rows(engines, what)
    finally:
        for eng in engines:
            eng.close()


# ---- the group's capacity refusal (run_group: in > r[4])
def _capacity_group(world, tpr, last):
    """epoch 1's batches: tpr txns of kMaxPos accesses from every origin,
    origin 0's last txn of `last`; the other epochs' batches: 2 accesses a txn"""
    M = K["kMaxPos"]
    cases = []
    for e in range(world):
        per = [[M - 2 if e == 1 else 0] * tpr for _ in range(world)]
        if e == 1:
            per[0][-1] = last - 2
        cases.append(A.ragged_ladder(A.arrange(per, "origin", tpr), 1, lambda k: k))
    return cases


def test_group_capacity_refusal():
    """Decider 1's capacity is one access short of its epoch's incoming
    batches (every sender within its own): DV_ERR_ARG on every rank, no row
    changes.  The next group brings it exactly its capacity and runs to the
    formula."""
    cc, world, tpr, M = "NO_WAIT", 3, 8, K["kMaxPos"]
    over = _capacity_group(world, tpr, M)
    fits = _capacity_group(world, tpr, M - 1)
    n_in = over[1].epoch.n_acc
    assert n_in == world * tpr * M and fits[1].epoch.n_acc == n_in - 1
    rows_pp = -(-max(c.rows for c in over + fits) // world)
    caps = [4 * n_in] * world
    caps[1] = n_in - 1
    engines = _engines(cc, world, rows_pp, tpr, caps, 2)
    table = _Table(rows_pp, world)
    try:
        for eng in engines:
            eng.set_prefix(None)
        homes = _homes(over, world, "origin", "start_bits")
        for r in range(world):  # every sender within its own capacity: the refusal is the decider's
            assert sum(h.n_acc for h in homes[r]) <= caps[r]
        assert sum(homes[r][1].n_acc for r in range(world)) == caps[1] + 1
        res = _run_group_epochs(engines, homes, tpr)
        for r, x in enumerate(res):
            assert isinstance(x, dvcc.DvccError) and x.code == dvcc._lib.DV_ERR_ARG, (r, x)
        table.check_rows(engines, "after the refused group")
        homes = _homes(fits, world, "origin", "start_bits")
        assert sum(homes[r][1].n_acc for r in range(world)) == caps[1]
        refs = [table.run(cc, case) for case in fits]
        res = _run_group_epochs(engines, homes, tpr)
        for r, x in enumerate(res):
            assert not isinstance(x, Exception), f"rank {r}: {x}"
        _check_group_result(cc, world, tpr, "origin", lambda r: res[r], refs, fits, "the fitting group")
        table.check_rows(engines, "after the fitting group")
    finally:
        for eng in engines:
            eng.close()
