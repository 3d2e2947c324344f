"""Prefix-kill epochs that carry their txn boundaries (dv_epoch_dev::txn_begin)
on a dense map keep no acc_row copy of their accesses: k_prefix_mark,
k_exec_txn and the route walk read the committed txns' row words from the
epoch's own records, and k_kill_emit takes a survivor's skipped accesses from
k_kill's skip bits.  Everything here is checked bit for bit against the CPU
oracle: commit bytes, committed count, read digest, write count and the whole
table; what the cases must contain (survivors, long committed survivors,
skipped reads) is computed from the oracle's commit bytes on the CPU."""
import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import CCEngine, DeviceEpoch, Epoch  # noqa: E402

ORACLE_CC = {dvcc.NO_WAIT: O.NO_WAIT, dvcc.WAIT_DIE: O.WAIT_DIE, dvcc.OCC: O.OCC}
ROWS, K, HOT = 1 << 12, 64, 16
LATER = (1, 512, 513, 1025)  # txns after the prefix: the kill tiles hold 512


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


def ragged_epoch(rows, n_txn, seed, longest=40, hot=HOT):
    """Ragged txns of 0..longest accesses: half of the accesses read one of
    the `hot` first rows (committed prefix readers leave those read-only, so
    survivors skip their reads of them), the others read or write a row drawn
    from the rest.  Row indices; the caller maps them to keys."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, longest + 1, size=n_txn)
    past = rng.random(n_txn) < 0.15  # (enough survivors past one skip word)
    lens[past] = rng.integers(33, longest + 1, size=int(past.sum()))
    tb = np.zeros(n_txn + 1, np.uint32)
    tb[1:] = np.cumsum(lens)
    n = int(tb[-1])
    is_hot = rng.random(n) < 0.5
    rws = np.where(is_hot, rng.integers(0, hot, size=n), rng.integers(hot, rows, size=n)).astype(np.uint64)
    types = np.where(is_hot, 0, rng.random(n) < 0.5).astype(np.uint8)
    return rws, types, tb


def survivors_of(cc, commit, rws, types, tb, k):
    """The later txns no committed prefix txn kills, and their accesses left
    after the skipped reads -- the rule of the engine's prefix kill, from the
    oracle's commit bytes: a committed prefix write kills every access of its
    row; under NO_WAIT / WAIT_DIE a committed prefix read kills a write of its
    row, and a read of a row that committed prefix txns only read is skipped."""
    nowait = cc != dvcc.OCC
    wr, rd = set(), set()
    for t in range(k):
        if commit[t]:
            for a in range(int(tb[t]), int(tb[t + 1])):
                (wr if types[a] else rd).add(int(rws[a]))
    surv, kept = [], 0
    for t in range(k, len(tb) - 1):
        acc = range(int(tb[t]), int(tb[t + 1]))
        if any(int(rws[a]) in wr or (nowait and types[a] and int(rws[a]) in rd) for a in acc):
            continue
        surv.append(t)
        kept += sum(1 for a in acc if not (nowait and not types[a] and int(rws[a]) in rd))
    return surv, kept


def epoch_facts(cc, commit, rws, types, tb, k):
    """(survivors, their accesses kept, their whole length, committed later
    txns longer than 32 accesses) of one epoch, from the oracle's commit bytes"""
    surv, kept = survivors_of(cc, commit, rws, types, tb, k)
    lens = np.diff(tb.astype(np.int64))
    long_committed = sum(1 for t in surv if lens[t] > 32 and commit[t])
    return len(surv), kept, int(sum(lens[t] for t in surv)), long_committed


def case_epochs(n_later, n_epochs=2):
    return [ragged_epoch(ROWS, K + n_later, 7000 + 10 * n_later + i) for i in range(n_epochs)]


def check_epoch(eng, cc, ix, f0, rows, keys, rws, types, tb, k, recs):
    """one epoch on the engine against the oracle; returns the oracle's commit bytes and the engine's stats"""
    e = Epoch(keys[rws.astype(np.int64)] if keys is not None else rws, types, tb)
    c_ref, _, st_ref = O.epoch_run(ORACLE_CC[cc], ix, f0, e.n_txn, e.txn_begin, e.keys, e.types)
    d = torch.zeros(e.n_txn, dtype=torch.uint8, device="cuda")
    dep = DeviceEpoch(e, txn_begin=True, recs32=recs)
    assert (dep.recs32 is not None) == recs
    st = eng.run_epoch_device(dep, d)
    assert st.prefix_txn == k, st.prefix_txn
    c = d.cpu().numpy()
    assert (c == c_ref[:e.n_txn]).all(), f"commit mismatch: {int((c != c_ref[:e.n_txn]).sum())} txns"
    assert (st.committed, st.read_digest, st.write_cnt) == (st_ref.committed, st_ref.read_digest, st_ref.write_cnt)
    assert (eng.read_table(0, rows) == f0).all(), "table mismatch"
    return c_ref, st


def test_cases_hold_on_the_oracle_alone():
    """(no engine) the seeds give what the cases below need, by the oracle's
    commit bytes: from 512 later txns on, every epoch has at least 32
    survivors, a committed later txn longer than 32 accesses and skipped
    reads; with one later txn, that txn survives."""
    for cc in ORACLE_CC:
        for n_later in LATER:
            for rws, types, tb in case_epochs(n_later):
                tab = O.YcsbTable(ROWS)
                c_ref, _, _ = O.epoch_run(ORACLE_CC[cc], tab.ix, tab.f0.copy(), len(tb) - 1, tb, rws, types)
                ns, kept, whole, long_committed = epoch_facts(cc, c_ref, rws, types, tb, K)
                if n_later == 1:
                    assert ns == 1, (cc, n_later)
                    continue
                assert ns >= 32 and long_committed >= 1, (cc, n_later, ns, long_committed)
                if cc != dvcc.OCC:  # (OCC skips nothing)
                    assert kept < whole, (cc, n_later)


@pytest.mark.parametrize("recs", [True, False])
@pytest.mark.parametrize("cc", list(ORACLE_CC))
@pytest.mark.parametrize("n_later", LATER)
def test_tile_and_word_edges(n_later, cc, recs):
    """1, 512, 513 and 1025 txns after a 64-txn prefix (one kill tile short,
    full, one over, two and one over), ragged txns of 0-40 accesses: empty
    txns, survivors on both sides of the 32-access skip word, ranges at any
    offset in a 64-access word of k_kill's bits.  Two epochs per engine, so
    stale workspace of the first would show in the second.  Each epoch with
    512 later txns or more has at least 32 survivors, one of them longer than
    32 accesses and committed, and (NO_WAIT / WAIT_DIE) skipped reads -- by
    the oracle's commit bytes, and the engine's survivor and sort-key counts
    are exactly those.  (One later txn cannot make 32 survivors: that case
    asks that the one txn survives.)"""
    epochs = case_epochs(n_later)
    tab = O.YcsbTable(ROWS)
    f0 = tab.f0.copy()
    eng = CCEngine(cc, K + n_later, max(int(tb[-1]) for _, _, tb in epochs))
    try:
        eng.load_ycsb_partition(ROWS)
        eng.set_prefix(K)
        for rws, types, tb in epochs:
            c_ref, st = check_epoch(eng, cc, tab.ix, f0, ROWS, None, rws, types, tb, K, recs)
            ns, kept, whole, long_committed = epoch_facts(cc, c_ref, rws, types, tb, K)
            print(f"n_later {n_later} cc {cc} recs {recs}: survivors {ns} kept {kept} of {whole} "
                  f"long committed {long_committed}; engine {st.surv_txn} / {st.surv_acc}")
            assert (st.surv_txn, st.surv_acc) == (ns, kept)
            if n_later == 1:
                assert ns == 1
                continue
            assert ns >= 32 and long_committed >= 1
            if cc != dvcc.OCC:
                assert st.surv_acc < whole
    finally:
        eng.close()


@pytest.mark.parametrize("recs", [True, False])
def test_chained_index_keeps_acc_row(recs):
    """A prefix epoch with txn_begin on a chained-index table (no dense map:
    k_kill / k_kill_emit probe the keys, the survivors' acc_row words are
    written as before and the execution reads them)."""
    rows, n_later = 2048, 700
    rng = np.random.default_rng(3)
    keys = rng.permutation(np.arange(rows, dtype=np.uint64) * 7 + 3)
    f0 = rng.integers(1, 2**63, size=rows, dtype=np.uint64)
    ix = O.MultiIndex(97, 1, 0, list(zip(keys.tolist(), range(rows))))
    rws, types, tb = ragged_epoch(rows, K + n_later, 7900)
    eng = CCEngine(dvcc.NO_WAIT, K + n_later, int(tb[-1]))
    try:
        eng.create_table(0, rows, 97, dvcc.HASH_MOD)
        eng.load_table(0, keys, f0)
        eng.set_prefix(K)
        c_ref, st = check_epoch(eng, dvcc.NO_WAIT, ix.ix, f0, rows, keys, rws, types, tb, K, recs)
        ns, kept, whole, _ = epoch_facts(dvcc.NO_WAIT, c_ref, rws, types, tb, K)
        assert (st.surv_txn, st.surv_acc) == (ns, kept)
        assert ns >= 32 and kept < whole
    finally:
        eng.close()


@pytest.mark.parametrize("cc", list(ORACLE_CC))
def test_committed_survivor_rows_execute(cc):
    """A later txn of 12 accesses on rows nobody else touches survives,
    commits and executes from its own records: the six rows it writes hold 0
    afterwards, the six it reads and the rows between them are untouched."""
    rws, types, tb = ragged_epoch(2048, K + 600, 7950)  # (the other txns stay below row 2048)
    t = K + 333
    own = 3000 + 3 * np.arange(12, dtype=np.uint64)  # 3000, 3003, ...: neighbours 3001, 3002, ... unused
    own_types = (np.arange(12) % 2).astype(np.uint8)
    a0, a1 = int(tb[t]), int(tb[t + 1])
    rws = np.concatenate([rws[:a0], own, rws[a1:]])
    types = np.concatenate([types[:a0], own_types, types[a1:]])
    tb = tb.copy()
    tb[t + 1:] = tb[t + 1:] - np.uint32(a1 - a0) + np.uint32(12)
    tab = O.YcsbTable(ROWS)
    f0 = tab.f0.copy()
    before = f0.copy()
    assert (before[2990:3050] != 0).all()
    eng = CCEngine(cc, K + 600, int(tb[-1]))
    try:
        eng.load_ycsb_partition(ROWS)
        eng.set_prefix(K)
        c_ref, st = check_epoch(eng, cc, tab.ix, f0, ROWS, None, rws, types, tb, K, True)
        assert c_ref[t] == 1
        got = eng.read_table(0, ROWS)
        written = own[own_types == 1].astype(np.int64)
        assert (got[written] == 0).all()
        rest = np.setdiff1d(np.arange(2990, 3050), written)
        assert (got[rest] == before[rest]).all()
    finally:
        eng.close()
