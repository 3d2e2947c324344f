"""The closed-form TPC-C epochs of tests/adversarial_tpcc.py on the HIP engine:
every family and algorithm through dv_tpcc_epoch_run_device, bit for bit
against the formula AND against the CPU oracle -- commit bytes, the o_id of
every txn, the committed and write counts, and all three columns of all five
tables after every epoch.

What the families reach in k_tpcc_apply / k_tpcc_oid (csrc/dvcc_tpcc.hip) that
a generated epoch does not: additive runs of 63 / 64 / 65 ... 1,025 accesses
that start mid-wave, a customer paid by id and by last name in one run,
district queues that end inside a step of 64, exactly on one and at n, stock
queues longer than a wave whose last write sits on either edge of the
S_QUANTITY rule, a grid sized by the commit bytes instead of the accesses,
queue starts left behind by earlier epochs (one lane, and two and four lanes
replaying captured graphs), and the grid-stride loop's second trip.
"""
import numpy as np
import pytest
import torch

import _oracle as O
import adversarial_tpcc as AT
import dvcc
from dvcc import tpcc as T

pytestmark = pytest.mark.gpu

CC = {"NO_WAIT": dvcc.NO_WAIT, "WAIT_DIE": dvcc.WAIT_DIE, "OCC": dvcc.OCC, "CALVIN": dvcc.CALVIN}
OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}
DECIDING = ("NO_WAIT", "WAIT_DIE", "OCC")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield
    AT.built_sweep.cache_clear()  # (the large epochs go with the module)


def _engine(case, cc, max_txn=None):
    return T.TpccEngine(CC[cc], case.cx.pp(), max_txn or AT.engine_max_txn(case), seed=AT.LOAD_SEED)


def _tables(db):
    return [db.table(t)[1:] for t in range(5)]


def _same_tables(eng, state, ref, what):
    """the engine's fifteen columns against the formula's and the oracle's"""
    for t in range(5):
        for col in range(3):
            got = eng.read_col(t, col)
            bad = np.flatnonzero(got != state[t][col])
            assert bad.size == 0, f"{what}: table {t} col {col} off the formula at rows {bad[:5]}"
            assert np.array_equal(got, ref[t][col]), f"{what}: table {t} col {col} off the oracle"


def _same_epoch(what, e, c, o, st, exp, ref):
    """one epoch's commit bytes, o_ids and counts against the formula (exp)
    and the oracle (ref)"""
    ec, eo, committed, wcnt = exp
    c_ref, o_ref, st_ref = ref
    assert np.array_equal(c, ec), f"{what}: {int((c != ec).sum())} commit bytes off the formula, first {np.flatnonzero(c != ec)[:8]}"
    assert np.array_equal(c, c_ref), f"{what}: commit bytes off the oracle"
    assert np.array_equal(o, eo), f"{what}: o_id off the formula at {np.flatnonzero(o != eo)[:8]}"
    assert np.array_equal(o, o_ref), f"{what}: o_id off the oracle"
    assert (st.committed, st.write_cnt) == (committed, wcnt), what
    assert (st.committed, st.write_cnt) == (st_ref.committed, st_ref.write_cnt), what


def _hold(case, cc):
    db = O.TpccDB(case.cx.po, AT.LOAD_SEED)
    state = case.cx.init()
    eng = _engine(case, cc)
    try:
        for k, e in enumerate(case.epochs):
            ec, eo, committed, wcnt, state = case.expect(cc, k, state)
            c_ref, o_ref, st_ref = db.epoch(OCC_ID[cc], e.keys, e.types, e.tables, e.args, e.txn_begin)
            dep, d_args = T.device_epoch(e)
            d_commit = torch.zeros(e.n_txn, dtype=torch.uint8, device="cuda")
            d_oid = torch.zeros(e.n_txn, dtype=torch.int64, device="cuda")
            st = eng.run_tpcc_epoch_device(dep, d_args, d_commit, d_oid)
            what = f"{cc} epoch {k}"
            _same_epoch(what, e, d_commit.cpu().numpy(), d_oid.cpu().numpy().view(np.uint64), st,
                        (ec, eo, committed, wcnt), (c_ref.copy(), o_ref.copy(), st_ref))
            _same_tables(eng, state, _tables(db), what)
    finally:
        eng.close()


@pytest.mark.parametrize("cc", AT.CCS)
@pytest.mark.parametrize("name", list(AT.CASES))
def test_family(name, cc):
    _hold(AT.built(name), cc)


# family 7: the only large one, once per algorithm and kind (cc is the fastest
# parameter: the four runs of a kind share its built epoch).  The oracle takes
# well under a second on it under every algorithm, WAIT_DIE included, so no
# family is shrunk for WAIT_DIE.
@pytest.mark.parametrize("cc", AT.CCS)
@pytest.mark.parametrize("kind", AT.SWEEPS)
def test_second_sweep(kind, cc):
    """4,096 x kBlock = 1,048,576 sorted accesses per sweep of k_tpcc_apply:
    the builder asserts that a customer's additive run (cust) / a stock queue
    (stock) straddles that index and that stock queue heads lie beyond it"""
    _hold(AT.built_sweep(kind), cc)


GRAPH_CALLS = 6


def _lanes_replayed(cases, cc, lanes):
    """the cases' epochs, in order, through run_tpcc_epochs_device over `lanes`
    decision lanes, GRAPH_CALLS calls from the same DeviceEpochs into the same
    buffers (as test_families_lanes_graph_replayed: plain twice, captured at
    the third call, replayed from the fourth), the tables carrying on from call
    to call: every epoch's commit bytes, o_ids and counts, and the tables after
    every call"""
    cx = cases[0].cx
    slots = [(case, k) for case in cases for k in range(len(case.epochs))]
    db = O.TpccDB(cx.po, AT.LOAD_SEED)
    state = cx.init()
    eng = _engine(cases[0], cc, max_txn=max(AT.engine_max_txn(c) for c in cases))
    try:
        extra = [eng.open_lane() for _ in range(lanes - 1)]
        devs = [T.device_epoch(case.epochs[k]) for case, k in slots]
        commits = [torch.zeros(case.epochs[k].n_txn, dtype=torch.uint8, device="cuda") for case, k in slots]
        oids = [torch.zeros(case.epochs[k].n_txn, dtype=torch.int64, device="cuda") for case, k in slots]
        for call in range(GRAPH_CALLS):
            sts = eng.run_tpcc_epochs_device([d for d, _ in devs], [a for _, a in devs], commits, oids, lanes=extra)
            for s, ((case, k), st) in enumerate(zip(slots, sts)):
                e = case.epochs[k]
                ec, eo, committed, wcnt, state = case.expect(cc, k, state)
                c_ref, o_ref, st_ref = db.epoch(OCC_ID[cc], e.keys, e.types, e.tables, e.args, e.txn_begin)
                _same_epoch(f"{cc} lanes {lanes} call {call} epoch {s}", e, commits[s].cpu().numpy(),
                            oids[s].cpu().numpy().view(np.uint64), st, (ec, eo, committed, wcnt),
                            (c_ref.copy(), o_ref.copy(), st_ref))
                commits[s].zero_()  # (the next call has to write every byte and o_id again)
                oids[s].zero_()
            _same_tables(eng, state, _tables(db), f"{cc} lanes {lanes} call {call}")
    finally:
        eng.close()


@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("cc", AT.CCS)
def test_district_queues_lanes_graph_replayed(cc, lanes):
    """family 3 (both variants, twice over: four epochs a call)"""
    a, b = AT.built("districts"), AT.built("districts_alone")
    _lanes_replayed([a, b, a, b], cc, lanes)


@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("cc", AT.CCS)
def test_stale_starts_lanes_graph_replayed(cc, lanes):
    """family 6: with two and four lanes every lane keeps queue starts of its
    own, several epochs old, and sees the three district sets in another
    order than the single lane does"""
    _lanes_replayed([AT.built("stale")], cc, lanes)


@pytest.mark.parametrize("cc", DECIDING)
def test_payment_storm_closed_loop(cc):
    """family 1 as the pool of dv_tpcc_epoch_run_closed_loop: 257 Payments on
    one warehouse, district and customer with h_j = j + 1, 100 txns an epoch.
    Every epoch commits exactly its oldest txn -- the carried ones come first,
    in pool order -- so epoch k applies pool txn k, after E epochs D_YTD has
    grown by E (E + 1) / 2, and the cursor stands at 100 + E.  The amounts
    travel in the op words: this pins that they stay with their txns through
    the carry."""
    N, E = 100, 12
    case = AT.built("storm_257")
    cx, pool = case.cx, case.epochs[0]
    h = case.extra["h"]
    assert np.array_equal(h, np.arange(1, 258, dtype=np.uint64)) and N + E <= pool.n_txn
    applied = np.zeros(pool.n_txn, np.uint8)
    applied[:E] = 1
    before = cx.init()
    _, after = AT._aggregate(cx, pool, applied, before)
    t, r = case.extra["rows"]["dist"]
    assert AT._f(after[t][0][r]) == AT._f(before[t][0][r]) + E * (E + 1) // 2
    eng = T.TpccEngine(CC[cc], cx.pp(), N, seed=AT.LOAD_SEED)
    try:
        dpool, pargs = T.device_epoch(pool)
        pb = torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        oids = [torch.zeros(N, dtype=torch.int64, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop(dpool, pargs, pb, N, E, d_commits=commits, d_oids=oids)
        only_first = np.zeros(N, np.uint8)
        only_first[0] = 1
        for k, st in enumerate(sts):
            assert np.array_equal(commits[k].cpu().numpy(), only_first), f"epoch {k}"
            assert not oids[k].cpu().numpy().any()
            assert (st.n_txn, st.committed, st.write_cnt) == (N, 1, 3), k
        assert int(cursor.item()) == N + E
        for tt in range(5):
            for col in range(3):
                assert np.array_equal(eng.read_col(tt, col), after[tt][col]), f"table {tt} col {col}"
        # the epoch left behind: pool txns E .. E + N - 1, in order, with their amounts
        nxt, nxt_args = bufs.epoch(E & 1, N, dpool.max_txn_acc)
        v = nxt_args.cpu().numpy().view(np.uint64) & np.uint64(AT.OP_MASK)
        assert np.array_equal(v, np.repeat(h[E:E + N], 3))
    finally:
        eng.close()
