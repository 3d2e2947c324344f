"""k_bucket_sort with one tag array in LDS and two workgroups per CU: parity
against the CPU oracle (commit bytes, Calvin grant groups, the F0 column, the
committed read digest) at the bucket sizes where the kernel changes path --
the wave, workgroup and step edges, the switch from LDS to global memory --
at one, two and three passes over the tag array, and under four decision
lanes (whose buckets share CUs)."""
import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import CCEngine, DeviceEpoch, Epoch, YCSBQueryGenerator  # noqa: E402

ORACLE_CC = {dvcc.NO_WAIT: O.NO_WAIT, dvcc.CALVIN: O.CALVIN}
HASH_MUL = 0x9E3779B1  # dvcc_internal.h kRowHashMul


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


def _run(cc, rows, epochs, prefix, tab=None):
    """test_gpu_parity's _check on the device path: every epoch's commit
    bytes, grant groups, counts and digest, and the table's F0 column after
    every epoch (tables past 2^24 rows: after the last one)"""
    tab = tab or O.YcsbTable(rows)
    f0 = tab.f0.copy()
    calvin = cc == dvcc.CALVIN
    eng = CCEngine(cc, max(e.n_txn for e in epochs), max(e.n_acc for e in epochs))
    try:
        eng.set_prefix(prefix)
        eng.load_ycsb_partition(rows)
        for k, e in enumerate(epochs):
            c_ref, g_ref, st_ref = O.epoch_run(ORACLE_CC[cc], tab.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types,
                                               want_grant=calvin)
            d_commit = torch.zeros(e.n_txn, dtype=torch.uint8, device="cuda")
            d_grant = torch.zeros(e.n_acc, dtype=torch.int32, device="cuda") if calvin else None
            st = eng.run_epoch_device(DeviceEpoch(e), d_commit, d_grant)
            c = d_commit.cpu().numpy()
            assert (c == c_ref).all(), f"epoch {k}: commit mismatch: {int((c != c_ref).sum())} txns"
            if calvin:
                g = d_grant.cpu().numpy().view(np.uint32)
                assert (g == g_ref).all(), f"epoch {k}: grant mismatch: {int((g != g_ref).sum())}"
            assert st.committed == st_ref.committed
            assert st.aborted == st_ref.aborted
            assert st.write_cnt == st_ref.write_cnt
            assert st.read_digest == st_ref.read_digest
            if prefix is not None and e.n_txn > prefix:
                assert st.prefix_txn, "prefix-kill path not taken"
            if rows <= 1 << 24 or k == len(epochs) - 1:
                assert (eng.read_table(0, rows) == f0).all(), f"epoch {k}: table state mismatch"
    finally:
        eng.close()


def _bucket_of(row, key_bits, lo):
    return ((row * HASH_MUL) & ((1 << key_bits) - 1)) >> (key_bits - lo)


def _same_bucket_rows(key_bits, lo, count=3):
    """`count` rows of one sort bucket, far apart in the bucket's order"""
    rows = np.arange(1 << key_bits, dtype=np.uint64)
    b = ((rows * np.uint64(HASH_MUL)) & np.uint64((1 << key_bits) - 1)) >> np.uint64(key_bits - lo)
    target = int(b[12345 % len(rows)])
    same = rows[b == target]
    assert len(same) >= count
    pick = same[np.linspace(0, len(same) - 1, count).astype(int)]
    assert all(_bucket_of(int(r), key_bits, lo) == target for r in pick)
    return pick


def _one_bucket_epoch(m, rows3, seed, p_write=0.3):
    """m one-access txns on rows that share a sort bucket: the bucket holds
    exactly m keys and every other bucket none; reads and writes mixed, so
    the row queues hold commits and aborts"""
    rng = np.random.default_rng(seed)
    keys = rows3[rng.integers(0, len(rows3), size=m)].astype(np.uint64)
    types = (rng.random(m) < p_write).astype(np.uint8)
    return Epoch(keys, types, np.arange(m + 1, dtype=np.uint32))


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 16383, 16384, 16385])
def test_exact_bucket_sizes(m):
    """one bucket of exactly m keys: a wave's 64, a step of 256 / 512 / 1,024
    threads, and 16,384 -- the most a workgroup sorts in LDS; one key more
    goes through global memory.  Whole epochs (NO_WAIT, CALVIN: the host knows
    the count) and prefix-kill stages (the counts are on the device)"""
    key_bits, lo = 16, 8
    rows3 = _same_bucket_rows(key_bits, lo)
    e = _one_bucket_epoch(m, rows3, 1000 + m)
    tab = O.YcsbTable(1 << key_bits)
    for cc in (dvcc.NO_WAIT, dvcc.CALVIN):
        _run(cc, 1 << key_bits, [e], None, tab)
    # mostly reads: the survivors' bucket stays near m
    e2 = _one_bucket_epoch(m, rows3, 2000 + m, p_write=0.02)
    _run(dvcc.NO_WAIT, 1 << key_bits, [e, e2], 7, tab)


def _hot_row_epoch(rows, n_txn, seed, R=4):
    """every txn reads one hot row first, then R - 1 random rows: the hot
    row's bucket holds more keys than a workgroup sorts in LDS"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, rows, size=(n_txn, R)).astype(np.uint64)
    keys[:, 0] = rows // 3
    types = (rng.random((n_txn, R)) < 0.5).astype(np.uint8)
    types[:, 0] = 0
    return Epoch(keys.reshape(-1), types.reshape(-1), (np.arange(n_txn + 1) * R).astype(np.uint32))


@pytest.mark.parametrize("log_rows", [16, 22, 26, "26+1", "27+1"])
def test_pass_counts(log_rows):
    """8, 14 and 18 row bits above the bucket digit: one, two and three passes
    over the single tag array (and over global memory for the hot row's
    20,000-key bucket), whole epochs and prefix-kill stages.  "26+1", "27+1":
    2^26 + 1 and 2^27 + 1 rows, which the runtime gives 27 and 28 key bits --
    512 and 1,024 buckets behind a hashed 9- and 10-bit first pass"""
    extra = 0
    if isinstance(log_rows, str):
        log_rows, extra = (int(x) for x in log_rows.split("+"))
    rows = (1 << log_rows) + extra
    g = YCSBQueryGenerator(rows, zipf_theta=0.9)
    eps = [g.gen(30_000, 151 + log_rows), _hot_row_epoch(rows, 20_000, 152 + log_rows)]
    tab = O.YcsbTable(rows)
    _run(dvcc.NO_WAIT, rows, eps, None, tab)
    _run(dvcc.NO_WAIT, rows, eps, 3000, tab)
    if log_rows <= 22:
        _run(dvcc.CALVIN, rows, eps, None, tab)


def test_two_workgroups_per_cu_under_lanes():
    """four decision lanes, each on its own quarter of the CUs, over a dozen
    140,000-txn prefix-kill epochs: every lane's bucket workgroups share CUs
    two by two; every commit buffer against the oracle"""
    rows, n_txn = 1 << 18, 140_000
    g = YCSBQueryGenerator(rows, zipf_theta=0.9)
    es = [g.gen(n_txn, dvcc.epoch_seed(3, k)) for k in range(12)]
    tab = O.YcsbTable(rows)
    f0 = tab.f0.copy()
    refs = [O.epoch_run(O.NO_WAIT, tab.ix, f0, n_txn, e.txn_begin, e.keys, e.types)[0] for e in es]
    eng = CCEngine(dvcc.NO_WAIT, n_txn, max(e.n_acc for e in es))
    lanes = []
    try:
        eng.load_ycsb_partition(rows)
        lanes = [eng.open_lane() for _ in range(3)]
        commits = [torch.zeros(n_txn, dtype=torch.uint8, device="cuda") for _ in es]
        sts = eng.run_epochs_lanes(lanes, [DeviceEpoch(e) for e in es], commits)
        for k, c_ref in enumerate(refs):
            c = commits[k].cpu().numpy()
            assert (c == c_ref).all(), f"lanes epoch {k}: commit mismatch: {int((c != c_ref).sum())} txns"
        assert all(st.prefix_txn for st in sts), "prefix-kill path not taken"
        assert (eng.read_table(0, rows) == f0).all(), "table state mismatch"
    finally:
        for ln in lanes:
            ln.close()
        eng.close()
