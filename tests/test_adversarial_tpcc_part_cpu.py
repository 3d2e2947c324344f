"""The partitioned closed-form TPC-C epochs (tests/adversarial_tpcc.py, family
8 and its shapes) without a GPU: what test_adversarial_tpcc_part_gpu.py hands
to dv_tpcc_epoch_run_part, checked against the CPU oracle and by arithmetic.

  * every shape, ownership and cut: the origins' batches (real n_txn, tables,
    operation words and owner bytes travelling along) sequenced again are the
    global epoch array for array, and O.TpccDB(index_parts=world).epoch(...,
    owner=...) over them equals the formula under all four algorithms --
    commit bytes, o_ids, counts and all fifteen columns;
  * owner_bytes (the partition from the warehouse in each key) equals the
    generator's own owner bytes on a generated epoch;
  * arithmetic from structural_constants() for the edges the shapes are named
    for -- the evidence that the GPU file reaches them:
      k_owner_count / k_owner_scan / k_owner_scatter   home batches of kTile - 1,
          kTile, kTile + 1 and 2 * kTile + 1 accesses (edges), one of 0, a
          33-access txn across the first tile edge, every owner's records in a
          tile b > 0; owners that receive everything private (part0) and
          nothing at all (skip_last, world 3: n_recv == 0)
      k_ilist_bounds / k_ilist_move / k_il_begin       position-major segments
          that start, end and are interleaved with txns without a record at the
          owner (equal starts under the lower bound); operation words moved with
          their records (model a)
      k_il_commits / k_il_words                        txns_per_rank 37 and 265 at
          world 3 (div_magic of values that are no power of two) carrying
          nonzero o_ids whose sequence number differs from their place in
          origin order (model b)
      k_max_reduce<uint64_t>                           o_ids computed on several
          partitions in one epoch (districts of different warehouses)
  * separation: numpy models of three wrong kernels, each shown to differ from
    the formula (test_model_*_is_separated).
"""
import numpy as np
import pytest

import _oracle as O
import adversarial as A
import adversarial_tpcc as AT
from adversarial_tpcc import T_CUST, T_DIST, T_STOCK
from dvcc import tpcc as T

OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}
ORDERS = ("origin", "position")
K = A.structural_constants()
KT = K["kOwnerTile"]
FIELDS = ("keys", "types", "tables", "args", "owner")
ALL = [(shape, world, own, order) for shape in AT.PART_SHAPES for world in AT.PART_WORLDS for own in A.OWNERSHIPS
       for order in ORDERS]


def _origin_order(v, world, tpr):
    return np.asarray(v).reshape(tpr, world).T.reshape(-1)


def _sequence(parts, tpr, order):
    """the origins' batches back in sequence order, txn by txn (each origin's
    missing slots empty txns): origin-major q * tpr + j, position-major
    j * world + q"""
    world = len(parts)
    slots = ([(q, j) for q in range(world) for j in range(tpr)] if order == "origin"
             else [(q, j) for j in range(tpr) for q in range(world)])
    cols = {f: [] for f in FIELDS}
    lens = []
    for q, j in slots:
        p = parts[q]
        a, b = (int(p.txn_begin[j]), int(p.txn_begin[j + 1])) if j < p.n_txn else (0, 0)
        lens.append(b - a)
        for f in FIELDS:
            cols[f].append(getattr(p, f)[a:b])
    tb = np.zeros(len(lens) + 1, np.uint32)
    tb[1:] = np.cumsum(lens)
    c = {f: np.concatenate(cols[f]) for f in FIELDS}
    return T.TpccEpoch(c["keys"], c["types"], tb, c["tables"], c["args"], None, c["owner"])


def _origin_of_txn(n_txn, world, tpr, order):
    t = np.arange(n_txn)
    return t // tpr if order == "origin" else t % world


@pytest.mark.parametrize("shape,world,own,order", ALL)
def test_cut_round_trips_and_oracle_holds(shape, world, own, order):
    case = AT.part_case(shape, world, own, order)
    tpr = case.extra["tpr"]
    dbs = {cc: O.TpccDB(case.cx.po, AT.LOAD_SEED, index_parts=world) for cc in AT.CCS}
    states = {cc: case.cx.init() for cc in AT.CCS}
    for k, e in enumerate(case.epochs):
        parts, tpr_ = AT.cut(e, world, order)
        assert tpr_ == tpr and tpr * world == e.n_txn
        for p in parts:  # (handed over with its real n_txn: no trailing empty txn)
            assert p.n_txn <= tpr and (p.n_txn == 0 or p.txn_begin[-1] > p.txn_begin[-2])
            assert all(len(getattr(p, f)) == p.n_acc for f in FIELDS)
        seq = _sequence(parts, tpr, order)
        assert np.array_equal(seq.txn_begin, e.txn_begin)
        for f in FIELDS:
            assert np.array_equal(getattr(seq, f), getattr(e, f)), f
        assert int(np.diff(e.txn_begin.astype(np.int64)).max()) <= AT.MAX_TXN_ACC
        for cc in AT.CCS:
            c, oid, committed, wcnt, states[cc] = case.expect(cc, k, states[cc])
            c_ref, o_ref, st = dbs[cc].epoch(OCC_ID[cc], seq.keys, seq.types, seq.tables, seq.args, seq.txn_begin,
                                             owner=seq.owner)
            assert np.array_equal(c_ref, c), f"{cc} epoch {k}: oracle and formula differ at {np.flatnonzero(c_ref != c)[:8]}"
            assert np.array_equal(o_ref, oid), f"{cc} epoch {k}: o_id"
            assert (st.committed, st.aborted, st.write_cnt) == (committed, e.n_txn - committed, wcnt), (cc, k)
            lad = case.extra["info"][k]["lad"]
            assert committed == e.n_txn - (0 if cc == "CALVIN" else len(lad) // 2)
            for t in range(5):
                ref = dbs[cc].table(t)
                for col in range(3):
                    assert np.array_equal(ref[1 + col], states[cc][t][col]), f"{cc} epoch {k}: table {t} col {col}"


@pytest.mark.parametrize("world", AT.PART_WORLDS)
def test_ycsb_cuts_unchanged_and_tpcc_cuts_agree(world):
    """the TPC-C cuts beside adversarial's: the same txn boundaries, keys and
    types as the YCSB functions give for the same epoch"""
    e = AT.part_case("mix", world, "spread", "origin").epochs[0]
    for order in ORDERS:
        mine, tpr = AT.cut(e, world, order)
        theirs, tpr_ = A.cut(e, world, order)
        assert tpr == tpr_
        for a, b in zip(mine, theirs):
            assert np.array_equal(a.txn_begin, b.txn_begin) and np.array_equal(a.keys, b.keys)
            assert np.array_equal(a.types, b.types)


@pytest.mark.parametrize("world", AT.PART_WORLDS)
def test_owner_bytes_match_the_generator(world):
    """owner_bytes against the owner bytes the generator writes (its own
    wh_to_part of the warehouse it drew): NewOrders with remote items"""
    cx = AT.ctx_world(world)
    p = O.tpcc_params(**dict(cx.kw, part_cnt=world, perc_payment=0.0))
    for home in range(world):
        keys, types, tables, args, tb, _, own = O.tpcc_gen(p, 200, 11 + home, home_part=home)
        e = T.TpccEpoch(keys, types, tb, tables, args)
        assert np.array_equal(AT.owner_bytes(cx, e, world), own)
        assert world == 1 or len(np.unique(own)) > 1


def _owner_view(p, world, tpr):
    """per owner: record count, home tiles of its records, txn slots with a record"""
    txn = p.acc_txn()
    out = []
    for o in range(world):
        at = np.flatnonzero(p.owner == o)
        has = np.zeros(tpr, bool)
        has[txn[at]] = True
        out.append((len(at), set((at // KT).tolist()), has))
    return out


def _runs_without(has):
    d = np.diff(np.r_[0, (~has).astype(np.int64), 0])
    return (np.flatnonzero(d == -1) - np.flatnonzero(d == 1)).tolist()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("own", A.OWNERSHIPS)
@pytest.mark.parametrize("world", AT.PART_WORLDS)
def test_edges_shape_reaches_the_owner_split_edges(world, own, order):
    """`edges`: the four epochs' big batches hold kTile - 1, kTile, kTile + 1
    and 2 * kTile + 1 accesses, one origin hands over nothing (n_home == 0), a
    33-access txn lies across the first tile edge of the 2 * kTile + 1 batch,
    every owner that is used has records in a home tile b > 0; part0 puts
    every private record on partition 0 (the others receive link and district
    records only: under 12 % of the epoch); skip_last leaves the last partition
    without private records and at world 3 without any record (n_recv == 0).
    Position-major, an origin with a small batch (9 of 265 slots) leaves every
    owner a segment that ends in 256 txns without a record."""
    assert KT == K["kXTile"] == 4096
    case = AT.part_case("edges", world, own, order)
    tpr = case.extra["tpr"]
    sizes, straddle, later = set(), 0, np.zeros(world, np.int64)
    for k, e in enumerate(case.epochs):
        parts, _ = AT.cut(e, world, order)
        assert sum(p.n_txn == 0 for p in parts) == 1 and sum(p.n_acc == 0 for p in parts) == 1
        big = max(parts, key=lambda p: p.n_acc)
        sizes.add(big.n_acc)
        tb, n = big.txn_begin.astype(np.int64), np.diff(big.txn_begin.astype(np.int64))
        if big.n_acc > KT:
            j = int(np.searchsorted(tb, KT, side="right")) - 1
            straddle += int(tb[j] < KT < tb[j + 1] and n[j] == AT.MAX_TXN_ACC)
        recv = np.zeros(world, np.int64)
        for p in parts:
            for o, (cnt, tiles, has) in enumerate(_owner_view(p, world, tpr)):
                recv[o] += cnt
                later[o] += bool(tiles - {0}) and p is big
                if order == "position" and cnt and 0 < p.n_txn < tpr // 2:
                    assert _runs_without(has)[-1] >= tpr - p.n_txn == 256
        assert int(recv.sum()) == e.n_acc
        if own == "part0":
            assert recv[0] > 0.88 * e.n_acc and recv[1:].min() > 0
        elif own == "skip_last" and world >= 3:
            assert recv[-1] == 0 and recv[:-1].min() > 0
        elif own == "skip_last":
            assert 0 < recv[-1] < 0.12 * e.n_acc  # (world 2: links alternate, so the last partition keeps its links)
        else:
            assert recv.min() > 0.25 * e.n_acc / world
    assert sizes == {KT - 1, KT, KT + 1, 2 * KT + 1}
    assert straddle == 1, "the 2 * kTile + 1 batch"
    used = world - 1 if (own == "skip_last" and world >= 3) else world
    assert (later[:used] >= 1).all(), "counts[o][b] with b > 0: every used owner, from the 2 * kTile + 1 batch"


@pytest.mark.parametrize("world", AT.PART_WORLDS)
def test_mix_shape_equal_starts(world):
    """`mix`, spread, position-major: txns_per_rank = 37 is no multiple of
    world or of 64, and every owner's segment from every origin holds txns
    without a record at that owner (empty txns, single accesses, 2-access
    ladder txns whose links live elsewhere): 8 to 25 of the 37, for every owner
    in runs of 2 to 6 from some origin; slot 0 of the first epoch is empty, so
    origin 0's segments start with one (tbo[0] == tbo[1] == 0), and at world 3
    seven segments end with one (at world 2 none does: there the edges shape's
    small batches do, test_edges_shape_reaches_the_owner_split_edges)."""
    case = AT.part_case("mix", world, "spread", "position")
    tpr = case.extra["tpr"]
    assert tpr == AT.MIX_TPR and tpr % world and tpr % 64
    first = last = 0
    longest = np.zeros(world, np.int64)
    for k, e in enumerate(case.epochs):
        parts, _ = AT.cut(e, world, "position")
        for q, p in enumerate(parts):
            for o, (cnt, tiles, has) in enumerate(_owner_view(p, world, tpr)):
                runs = _runs_without(has)
                assert cnt > 0 and 8 <= sum(runs) <= 25
                longest[o] = max(longest[o], max(runs))
                first += not has[0]
                last += not has[-1]
        if k == 0:
            assert all(not has[0] for _, _, has in _owner_view(parts[0], world, tpr))
    assert (longest >= 2).all() and longest.max() == (3 if world == 2 else 6)
    assert first >= world and last == (0 if world == 2 else 7)


@pytest.mark.parametrize("shape,world,own,order", ALL)
def test_o_ids_come_from_several_partitions(shape, world, own, order):
    """the district accesses: at least two warehouses' districts hand out
    o_ids in every epoch (the MAX all-reduce has something to combine), one
    district three of them under CALVIN (+ 1, + 2, + 3) and one otherwise"""
    case = AT.part_case(shape, world, own, order)
    cx = case.cx
    state = {cc: cx.init() for cc in ("OCC", "CALVIN")}
    for k, e in enumerate(case.epochs):
        nod = e.tables == T_DIST
        assert len(np.unique(e.owner[nod])) >= 2
        for cc in state:
            before = state[cc]
            c, oid, _, _, state[cc] = case.expect(cc, k, before)
            d0 = case.extra["info"][k]["dist"][0]
            txns = e.acc_txn()[nod & (e.keys == d0)]
            first = int(before[T_DIST][1][int(cx.row(T_DIST, d0))])
            assert len(txns) == 3
            got = sorted(int(oid[t]) for t in txns)
            assert got == ([first + 1, first + 2, first + 3] if cc == "CALVIN" else [0, 0, first + 1])


# ---- separation: the formula against numpy models of three wrong kernels
def _late_words(case, k, order):
    """model (a): the operation words arrive one record late inside every
    received segment (records of one origin at one owner, in batch order): the
    first record of a segment gets no word, every other its predecessor's.  A
    word that then names another table is ignored, as k_tpcc_apply does."""
    e = case.epochs[k]
    world, tpr = case.extra["world"], case.extra["tpr"]
    origin = _origin_of_txn(e.n_txn, world, tpr, order)[e.acc_txn()]
    args = e.args.copy()
    for q in range(world):
        for o in range(world):
            at = np.flatnonzero((origin == q) & (e.owner == o))
            if at.size:
                args[at[1:]] = e.args[at[:-1]]
                args[at[0]] = 0
    op = args >> np.uint64(56)
    table_of = np.array([255, AT.T_WH, T_DIST, T_CUST, T_DIST, T_STOCK], np.uint8)
    args[table_of[op] != e.tables] = 0
    return T.TpccEpoch(e.keys, e.types, e.txn_begin, e.tables, args, None, e.owner)


def _differs(a, b):
    return any(not np.array_equal(a[t][col], b[t][col]) for t in range(5) for col in range(3))


@pytest.mark.parametrize("shape,world,own,order", ALL)
def test_model_late_words_is_separated(shape, world, own, order):
    case = AT.part_case(shape, world, own, order)
    before = case.cx.init()
    for cc in ("NO_WAIT", "CALVIN"):
        c, oid, _, _, after = case.expect(cc, 0, before)
        wrong_oid, wrong = AT._aggregate(case.cx, _late_words(case, 0, order), c, before)
        assert _differs(wrong, after), "words one record late are not told apart"
        for t in (T_CUST, T_STOCK):  # (operands are distinct: both tables show it)
            assert not np.array_equal(wrong[t][1], after[t][1])


@pytest.mark.parametrize("shape", AT.PART_SHAPES)
@pytest.mark.parametrize("own", A.OWNERSHIPS)
@pytest.mark.parametrize("world", AT.PART_WORLDS)
def test_model_oid_in_sequence_order_is_separated(shape, world, own):
    """model (b): k_il_words left out -- the o_ids stay by sequence number
    (j * world + q) where the caller reads origin order (q * tpr + j).  Told
    apart at world 2 and at world 3, in every epoch."""
    case = AT.part_case(shape, world, own, "position")
    tpr = case.extra["tpr"]
    state = case.cx.init()
    for k in range(len(case.epochs)):
        _, oid, _, _, state = case.expect("OCC", k, state)
        want = _origin_order(oid, world, tpr)
        assert (oid != 0).sum() >= 3 and not np.array_equal(oid, want), (world, k)
        # (nor is a transposition the other way round right)
        assert not np.array_equal(oid.reshape(world, tpr).T.reshape(-1), want)


def _local_verdicts(case, k):
    """model (c): no verdict combine -- every partition decides its own records
    alone in sequence order (a txn loses at a partition when an earlier txn
    that won THERE wrote one of its rows there) and applies what won there.
    Returned as an epoch of world sub-txns per txn with their commit bytes."""
    e = case.epochs[k]
    world = case.extra["world"]
    txn = e.acc_txn()
    order = np.lexsort((np.arange(e.n_acc), e.owner, txn))  # by txn, then owner, stable
    sub = (txn.astype(np.int64) * world + e.owner)[order]
    lens = np.bincount(sub, minlength=e.n_txn * world)
    tb = np.zeros(len(lens) + 1, np.uint32)
    tb[1:] = np.cumsum(lens)
    split = T.TpccEpoch(e.keys[order], e.types[order], tb, e.tables[order], e.args[order], None, e.owner[order])
    rows = (split.tables.astype(np.int64) << 40) | split.keys.astype(np.int64)
    held, c = set(), np.ones(len(lens), np.uint8)
    for s in range(len(lens)):
        mine = rows[tb[s]:tb[s + 1]].tolist()
        if any(r in held for r in mine):
            c[s] = 0
        else:
            held.update(mine)
    return split, c


@pytest.mark.parametrize("shape,world,own,order", ALL)
def test_model_local_verdicts_is_separated(shape, world, own, order):
    """a txn that lost on the partition of one link is still applied on the
    others: rows of aborted txns change (the private rows of the odd ladder
    txns, used once: their final value names the txn)"""
    case = AT.part_case(shape, world, own, order)
    before = case.cx.init()
    c, _, _, _, after = case.expect("NO_WAIT", 0, before)
    split, c_local = _local_verdicts(case, 0)
    lost = np.flatnonzero(c == 0)
    assert lost.size and c_local.reshape(-1, world)[lost].any(), "no aborted txn wins anywhere on its own"
    _, wrong = AT._aggregate(case.cx, split, c_local, before)
    assert _differs(wrong, after)
    assert not np.array_equal(wrong[T_CUST][1], after[T_CUST][1])


# ---- the single-context families as test_family_part hands them over (world 2)
@pytest.mark.parametrize("name", AT.PART_CASES)
def test_families_cut_for_two_partitions(name):
    """every epoch padded to an even txn count, its owner bytes from the keys,
    both cuts sequenced again; the oracle with per-partition last-name lists
    and these owner bytes still equals the formula (the padding txn commits).
    Which families put records on both partitions is stated at the end."""
    world = 2
    case = AT.built(name)
    cx = case.cx
    assert cx.kw["num_wh"] == world
    both = 0
    for cc in AT.CCS:
        db = O.TpccDB(cx.po, AT.LOAD_SEED, index_parts=world)
        state = cx.init()
        for k, e in enumerate(case.epochs):
            tpr = -(-e.n_txn // world)
            full = AT.padded(e, tpr * world)
            full.owner = AT.owner_bytes(cx, e, world)
            both += len(np.unique(full.owner)) == world
            if cc == "CALVIN":
                for order in ORDERS:
                    parts, tpr_ = AT.cut(full, world, order)
                    seq = _sequence(parts, tpr, order)
                    assert tpr_ == tpr and np.array_equal(seq.txn_begin, full.txn_begin)
                    assert all(np.array_equal(getattr(seq, f), getattr(full, f)) for f in FIELDS)
            c, oid, committed, wcnt, state = case.expect(cc, k, state)
            pad = tpr * world - e.n_txn
            c_ref, o_ref, st = db.epoch(OCC_ID[cc], full.keys, full.types, full.tables, full.args, full.txn_begin,
                                        owner=full.owner)
            assert np.array_equal(c_ref, np.r_[c, np.ones(pad, np.uint8)])
            assert np.array_equal(o_ref, np.r_[oid, np.zeros(pad, np.uint64)])
            assert (st.committed, st.write_cnt) == (committed + pad, wcnt)
    # fillers sit on warehouse 1 beside a storm on warehouse 2, the sparse
    # carriers and the stale starts' eighteen districts span both; every other
    # family keeps to one warehouse: one partition receives every record, the
    # other none (n_recv == 0)
    spans = "_fill" in name or name == "storm_65_rdwh" or name == "stale" or name.startswith("sparse")
    assert bool(both) == spans, name
