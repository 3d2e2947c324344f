"""The closed-form index tables of tests/index_cases.py through every kernel
that inlines probe_row: k_gather_rows (read_rows), k_probe<false> (host
records and device epochs, with the prefix's pair_limit branch), k_probe_tb /
k_kill / k_kill_emit (epochs with their txn boundaries, as keys + types and as
4-byte records), the LDS descriptor copy of epochs that name tables,
k_probe_hist, the lanes over the owner's frozen tables and the replicated
branch.  Rows, commit bytes, counts, digests, the F0 column and error codes
are all compared exactly: with `where` (built from the insertion order), with
the formulas of index_cases.py and with the CPU oracle, which
test_index_cases_cpu.py holds to both.
"""
import functools

import numpy as np
import pytest
import torch

import _oracle as O
import index_cases as I
import dvcc
from dvcc import CCEngine, DeviceEpoch
from test_partitioned import _engine_group, _run_group

pytestmark = pytest.mark.gpu

CC = {"NO_WAIT": dvcc.NO_WAIT, "WAIT_DIE": dvcc.WAIT_DIE, "OCC": dvcc.OCC, "CALVIN": dvcc.CALVIN}
OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}
DECIDING = ("NO_WAIT", "WAIT_DIE", "OCC")
K = I.structural_constants()
PV = K["kPV"]
ERR_KEY, ERR_TABLE = dvcc._lib.DV_ERR_KEY_NOT_FOUND, dvcc._lib.DV_ERR_NO_TABLE
NAMES = I.case_names()
TABLE_FORMS = [n for n in NAMES if I.case(n).form == "table"]
PREFIX_K = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield
    for f in (_seq_ref, _good_ref, _tb_ref, _hist_ref):
        f.cache_clear()  # (the shared references go with the module)


def _engine(c, cc, max_txn=1024, max_acc=8192, table=0, dense0=0):
    eng = CCEngine(CC[cc], max_txn, max_acc, part_cnt=c.part_cnt, part_id=c.part_id)
    if dense0:
        eng.load_ycsb_partition(dense0)
    if c.form == "ycsb":
        eng.load_ycsb_partition(c.rows)
    else:
        eng.create_table(table, c.rows, c.nbuckets, c.hash_kind)
        eng.load_table(table, np.array(c.keys, dtype=np.uint64), c.f0[:c.n])
    return eng


def _oracle(t, f0, cc, e):
    """the oracle over e on f0 (changed in place): commit bytes and counts"""
    c, _, st = O.epoch_run(OCC_ID[cc], t.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types)
    return c.copy(), (st.committed, st.aborted, st.write_cnt, st.read_digest)


def _counts(st):
    return (st.committed, st.aborted, st.write_cnt, st.read_digest)


def _host(eng, e):
    c, _, st = eng.run_epoch(e)
    return c, st


def _dev(eng, e, **kw):
    dep = DeviceEpoch(e, **kw)
    d = torch.zeros(max(1, e.n_txn), dtype=torch.uint8, device="cuda")
    st = eng.run_epoch_device(dep, d)
    return d.cpu().numpy()[:e.n_txn], st


def _dev_acc(eng, e):
    return _dev(eng, e, txn_begin=False)


def _rejected(call, code=ERR_KEY, what=""):
    with pytest.raises(dvcc.DvccError) as ex:
        call()
    assert ex.value.code == code, (what, ex.value.code)


# ---------------------------------------------------------------- the two epochs, in closed form
@functools.lru_cache(maxsize=None)
def _seq_ref(name, cc):
    c = I.case(name)
    t, f0, out = I.oracle_table(c), c.f0.copy(), []
    for ec in (I.read_epoch(c), I.write_epoch(c), I.pair_epoch(c)):
        commit, counts = _oracle(t, f0, cc, ec.epoch)
        out.append((ec, commit, counts, f0.copy()))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_read_write_and_pair_epochs(name):
    """The read epoch (one reader per present key, then a writer of a read
    key), the write epoch (one writer per present key) and the pairs (two
    keys of one bucket; one key twice): commit bytes by the formula, counts
    and digest the oracle's, F0 the initial column with zero exactly at
    where[key] of the committed writes."""
    c = I.case(name)
    for cc in I.CCS:
        eng = _engine(c, cc)
        try:
            assert np.array_equal(eng.read_table(0, c.rows), c.f0), (cc, "the loaded column")
            written = []
            for run, (ec, c_ref, counts, f0) in zip((_host, _dev, _dev_acc), _seq_ref(name, cc)):
                got, st = run(eng, ec.epoch)
                assert got.shape == ec.expected[cc].shape
                assert np.array_equal(got, ec.expected[cc]), (cc, run.__name__, "off the formula")
                assert np.array_equal(got, c_ref) and _counts(st) == counts, (cc, run.__name__, "off the oracle")
                written += ec.written[cc]
                col = eng.read_table(0, c.rows)
                assert np.array_equal(col, I.column_after(c, written)) and np.array_equal(col, f0), (cc, run.__name__)
            assert _seq_ref(name, cc)[1][2][2] == len(c.present_keys())  # (write_cnt of the write epoch)
        finally:
            eng.close()


# ---------------------------------------------------------------- 1. read_rows (k_gather_rows)
@pytest.mark.parametrize("name", NAMES)
def test_read_rows(name):
    """Every key of the table returns its own row's F0 (a distinct value per
    row), in one call of a length that leaves a scalar tail and in calls of
    1 .. kPV keys; every missing probe, alone and in the middle of present
    keys, is DV_ERR_KEY_NOT_FOUND and the next call is right again."""
    c = I.case(name)
    eng = _engine(c, "NO_WAIT")
    try:
        keys = list(c.where)
        want = np.array([c.f0[c.where[k]] for k in keys], np.uint64)
        assert np.array_equal(eng.read_rows(np.array(keys, dtype=np.uint64)), want)
        ks = c.present_keys()
        pw = np.array([c.f0[c.where[k]] for k in ks], np.uint64)
        for n in range(1, min(len(ks), PV + 1) + 1):
            assert np.array_equal(eng.read_rows(np.array(ks[:n], dtype=np.uint64)), pw[:n])
        for lab, k in c.missing:
            _rejected(lambda: eng.read_rows(np.array([k], dtype=np.uint64)), what=lab)
            if ks:
                mid = ks[:PV + 1] + [k] + ks[:2]
                _rejected(lambda: eng.read_rows(np.array(mid, dtype=np.uint64)), what=lab)
                assert np.array_equal(eng.read_rows(np.array(ks, dtype=np.uint64)), pw), lab
        assert np.array_equal(eng.read_table(0, c.rows), c.f0)
    finally:
        eng.close()


# ---------------------------------------------------------------- 2, 3. flat epochs through k_probe<false>
@functools.lru_cache(maxsize=None)
def _good_ref(name, cc, n_acc):
    """single-access txns reading every present key, padded to n_acc accesses: all commit"""
    c = I.case(name)
    e = I.pad_epoch(c, c.present_keys(), n_acc)
    commit, counts = _oracle(I.oracle_table(c), c.f0.copy(), cc, e)
    assert commit.all() and counts[2] == 0
    return e, commit, counts


def _base(c):
    """the present keys and one pad, rounded up to whole kPV-wide vectors, past the prefix"""
    return max(PV * -(-(len(c.present_keys()) + 1) // PV), 4 * PV)


def _layouts(padded=True):
    """(place, index of the probe, accesses) of a flat epoch: the first
    access; the last one, in a whole vector; a lane in the middle of a
    kPV-wide vector; the scalar tail.  Without a key to pad with, the one
    access."""
    if not padded:
        return [("only", 0, 1)]
    n = 4 * PV
    return [("first", 0, n), ("last", n - 1, n), ("mid-vector", n - PV + 1, n + 1), ("tail", n + 1, n + 3)]


def _flat_consumer(name, run, ccs, prefix):
    """present keys with n_acc % kPV = 0 .. 3 under every algorithm of `ccs`,
    then every missing probe at every place (the algorithm in turn): the
    epoch is rejected, the table unchanged and the next good epoch bit-exact"""
    c = I.case(name)
    engines = {}

    def good(eng, cc, n_acc, what):
        if not c.present:  # (no key, no good epoch but the empty one)
            return
        e, c_ref, counts = _good_ref(name, cc, n_acc)
        got, st = run(eng, e)
        assert np.array_equal(got, c_ref) and _counts(st) == counts, (cc, what)
        if prefix and cc != "CALVIN":
            assert st.prefix_txn == prefix, (cc, what, st.prefix_txn)
        assert np.array_equal(eng.read_table(0, c.rows), c.f0), (cc, what)
    try:
        for cc in ccs:
            eng = engines[cc] = _engine(c, cc)
            eng.set_prefix(prefix)
            for rem in range(PV):
                good(eng, cc, _base(c) + rem, f"n_acc % kPV = {rem}")
        for i, (lab, k) in enumerate(c.missing):
            cc = ccs[i % len(ccs)]
            eng = engines[cc]
            for place, at, n in _layouts(bool(c.present)):
                _rejected(lambda: run(eng, I.flat_epoch(c, n, at, k)), what=(cc, lab, place))
                assert np.array_equal(eng.read_table(0, c.rows), c.f0), (cc, lab, place)
                good(eng, cc, _base(c), (lab, place, "the next good epoch"))
    finally:
        for eng in engines.values():
            eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_host_records(name):
    """run_epoch: k_split_access and k_probe<false>, all four algorithms"""
    _flat_consumer(name, _host, I.CCS, None)


@pytest.mark.parametrize("prefix", [None, PREFIX_K], ids=["prefix_off", "prefix_8"])
@pytest.mark.parametrize("name", NAMES)
def test_device_epochs_without_boundaries(name, prefix):
    """run_epoch_device over acc_txn; with set_prefix(8) the probe's
    pair_limit branch (CALVIN takes no prefix)"""
    _flat_consumer(name, _dev_acc, I.CCS if prefix is None else DECIDING, prefix)


# ---------------------------------------------------------------- 4. k_probe_tb, k_kill, k_kill_emit
def _tb_epoch(c, miss=None, place=None):
    """PREFIX_K prefix txns -- [W H], then the present keys read in up to 7
    txns -- and a few dozen later ones: per chunk one txn that reads it and
    then H (the prefix wrote H: killed) and one that reads it alone (a
    survivor), then 10 single reads.  miss: a key put in the middle of the
    first chunk's txn of `place`."""
    ks = c.present_keys()
    H, probes = ks[-1], ks[:-1] or ks
    chunks = [ch for ch in (probes[i::PREFIX_K - 1] for i in range(PREFIX_K - 1)) if ch]

    def reads(ch, where):
        ch = list(ch)
        if miss is not None and where == place and ch[0] == chunks[0][0]:
            ch.insert((len(ch) + 1) // 2, miss)
        return [(k, I.RD) for k in ch]
    txns = [[(H, I.WR)]] + [reads(ch, "prefix") for ch in chunks]
    txns += [[(ks[0], I.RD)]] * (PREFIX_K - len(txns))
    assert len(txns) == PREFIX_K
    for ch in chunks:
        txns.append(reads(ch, "killed") + ([(H, I.RD)] if H not in ch else []))
        txns.append(reads(ch, "survivor"))
    txns += [[(ks[0], I.RD)]] * 10
    return I._mk(txns)


@functools.lru_cache(maxsize=None)
def _tb_ref(name, cc):
    c = I.case(name)
    t, f0 = I.oracle_table(c), c.f0.copy()
    e = _tb_epoch(c)
    commit, counts = _oracle(t, f0, cc, e)
    good = I.flat_epoch(c, 3 * PV + 1)
    g_commit, g_counts = _oracle(t, f0, cc, good)  # (reads only: f0 stays)
    return e, commit, counts, f0, good, g_commit, g_counts


def _fits(k):
    return k < (1 << 31)


# (a table without keys has no prefix to form; 4-byte records hold keys below
# 2^31 -- Epoch.to_row_records refuses others, so those cases have no such epoch)
TB_NAMES = [n for n in NAMES if I.case(n).present]
RECS_NAMES = [n for n in TB_NAMES if all(_fits(k) for k in I.case(n).present_keys())]


@pytest.mark.parametrize("name", TB_NAMES)
def test_epochs_with_txn_boundaries(name):
    """set_prefix(8) and the epoch's own txn_begin, accesses as keys + types:
    the prefix's keys are probed by k_probe_tb, a killed later txn's by k_kill
    and a survivor's by k_kill_emit.  Every present key stands in all three;
    every missing probe is put in each in turn."""
    _tb_consumer(name, False)


@pytest.mark.parametrize("name", RECS_NAMES)
def test_epochs_with_txn_boundaries_recs32(name):
    """the same with the accesses as 4-byte records (keys below 2^31)"""
    _tb_consumer(name, True)


def _tb_consumer(name, recs):
    c = I.case(name)
    fits = _fits
    for i, cc in enumerate(DECIDING):
        eng = _engine(c, cc)
        try:
            eng.set_prefix(PREFIX_K)
            e, c_ref, counts, f0, good, g_commit, g_counts = _tb_ref(name, cc)

            def run(ep):
                dep = DeviceEpoch(ep, txn_begin=True, recs32=recs)
                assert (dep.recs32 is not None) == recs
                d = torch.zeros(ep.n_txn, dtype=torch.uint8, device="cuda")
                st = eng.run_epoch_device(dep, d)
                assert st.prefix_txn == PREFIX_K, st.prefix_txn
                return d.cpu().numpy(), st
            got, st = run(e)
            assert np.array_equal(got, c_ref) and _counts(st) == counts, cc
            if len(c.present_keys()) > 1:
                assert st.surv_txn > 0, "no survivor: k_kill_emit probed nothing"
            assert np.array_equal(eng.read_table(0, c.rows), f0), cc
            for j, (lab, k) in enumerate(c.missing):
                if j % len(DECIDING) != i or (recs and not fits(k)):
                    continue
                for place in ("prefix", "killed", "survivor"):
                    _rejected(lambda: run(_tb_epoch(c, k, place)), what=(cc, lab, place))
                    assert np.array_equal(eng.read_table(0, c.rows), f0), (cc, lab, place)
                    got, st = run(good)
                    assert np.array_equal(got, g_commit) and _counts(st) == g_counts, (cc, lab, place)
        finally:
            eng.close()


def _launched(eng, call):
    """the kernels `call` launches (dv_kernel_times)"""
    eng.set_timing(False, profile=True)
    eng.kernel_times()
    call()
    names = set(eng.kernel_times())
    eng.set_timing(False)
    return names


def test_each_consumer_launches_its_probe_kernel():
    """what the consumers above are there to reach, on a chained table: host
    records and device epochs k_probe (with a prefix, k_kill and k_kill_emit
    over its acc_row words), epochs with their boundaries k_probe_tb, k_kill
    and k_kill_emit over keys, in both forms"""
    c = I.case("CH_mod_97")
    eng = _engine(c, "NO_WAIT")
    try:
        assert "k_probe" in _launched(eng, lambda: _host(eng, I.flat_epoch(c, 4 * PV + 3)))
        eng.set_prefix(PREFIX_K)
        assert {"k_probe", "k_kill", "k_kill_emit"} <= _launched(eng, lambda: _dev_acc(eng, I.flat_epoch(c, 4 * PV + 3)))
        for recs in (False, True):
            got = _launched(eng, lambda: _dev(eng, _tb_epoch(c), txn_begin=True, recs32=recs))
            assert {"k_probe_tb", "k_kill", "k_kill_emit"} <= got and "k_probe" not in got, (recs, got)
    finally:
        eng.close()


# ---------------------------------------------------------------- 5. epochs that name tables (s_td)
DENSE0 = 1 << 20


@pytest.mark.parametrize("table", [1, K["kMaxTables"] - 1], ids=["table_1", "last_table"])
@pytest.mark.parametrize("name", TABLE_FORMS)
def test_beside_a_dense_table(name, table):
    """The case's table as table 1 / kMaxTables - 1 beside a dense table 0 of
    2^20 rows (row_base above 2^20), in epochs that name their tables: rows,
    digest (by the formula over where[key]) and both tables' columns; missing
    keys at every place; a table id one past the last created one and id 255
    are DV_ERR_NO_TABLE."""
    c = I.case(name)
    P, part = c.part_cnt, c.part_id
    ks = c.present_keys()
    k0 = [0 * P + part, (DENSE0 - 1) * P + part]           # table 0's first and last key
    w0 = 5 * P + part
    rd = [(k, table) for k in ks[:-1]] + [(k, 0) for k in k0]
    rd = rd[0::2] + rd[1::2]                                # (the tables mixed)
    wr = ([(ks[-1], table)] if ks else []) + [(w0, 0)]

    def epoch(accs, n_rd):
        return I._mk([[(k, I.RD if i < n_rd else I.WR)] for i, (k, _) in enumerate(accs)],
                     tables=np.array([t for _, t in accs], np.uint8))
    value = lambda k, t: I.ycsb_f0(k) if t == 0 else int(c.f0[c.where[k]])  # noqa: E731
    digest = I.read_digest([value(k, t) for k, t in rd], range(len(rd)), [k for k, _ in rd])
    for cc, run in (("NO_WAIT", _dev), ("OCC", _host)):
        eng = _engine(c, cc, table=table, dense0=DENSE0)
        try:
            def unchanged(written, what, w0_done=True):
                assert np.array_equal(eng.read_table(0, c.rows, table=table), I.column_after(c, written)), what
                col0 = eng.read_table(0, 16, table=0)
                assert [int(x) for x in col0] == [0 if w0_done and r * P + part == w0 else I.ycsb_f0(r * P + part)
                                                  for r in range(16)], what
                assert int(eng.read_table(DENSE0 - 1, 1, table=0)[0]) == I.ycsb_f0(k0[1]), what

            def good(what):
                got, st = run(eng, epoch(rd, len(rd)))
                assert got.all() and _counts(st) == (len(rd), 0, 0, digest), (cc, what)
            good("reads")
            unchanged([], "reads", w0_done=False)
            got, st = run(eng, epoch(rd + wr, len(rd)))
            assert got.all() and _counts(st) == (len(rd) + len(wr), 0, len(wr), digest), cc
            done = ks[-1:]
            unchanged(done, "writes")
            if ks:
                assert np.array_equal(eng.read_rows(np.array(ks, dtype=np.uint64), table=table),
                                      I.column_after(c, done)[[c.where[k] for k in ks]])
            pad = (k0[0], 0)
            for lab, k in c.missing:
                for place, at, n in _layouts():
                    accs = [pad] * n
                    accs[at] = (k, table)
                    _rejected(lambda: run(eng, epoch(accs, n)), what=(cc, lab, place))
                    unchanged(done, (lab, place))
                good((lab, "the next good epoch"))
            for bad in (table + 1, 255):
                accs = [pad] * (2 * PV) + [(k0[0], bad)] + [pad] * 2
                _rejected(lambda: run(eng, epoch(accs, len(accs))), ERR_TABLE, what=(cc, bad))
                unchanged(done, bad)
            good("after the table errors")
        finally:
            eng.close()


# ---------------------------------------------------------------- 6. k_probe_hist
HIST_N = K["kProbeHistTiles"] * K["kTile"]
HIST_LEN = 16


def _hist_epoch(c, n_acc, last=None):
    """read-only txns of HIST_LEN accesses cycling a short list of present
    keys (the last txn shorter / one access long); `last`: the key of the
    very last access"""
    short = _short_rows(c)
    ks = [k for k in c.present_keys() if c.where[k] in short]
    ks = ks[:HIST_LEN // 2] + ks[-(HIST_LEN // 2):] if len(ks) > HIST_LEN else ks
    keys = np.resize(np.array(ks, dtype=np.uint64), n_acc)
    if last is not None:
        keys[-1] = np.uint64(last)
    tb = np.minimum(np.arange(0, n_acc + HIST_LEN, HIST_LEN), n_acc).astype(np.uint32)
    if tb[-1] == tb[-2]:
        tb = tb[:-1]
    return dvcc.Epoch(keys, np.zeros(n_acc, np.uint8), tb)


def _short_rows(c):
    """rows of keys in chains of at most 65 entries (the oracle walks a chain per access)"""
    per = {}
    for k in c.where:
        per.setdefault(c.bucket(k), []).append(k)
    return {c.where[k] for b, ch in per.items() if len(ch) <= 65 for k in ch}


@functools.lru_cache(maxsize=None)
def _hist_ref(name, n_acc):
    c = I.case(name)
    e = _hist_epoch(c, n_acc)
    commit, counts = _oracle(I.oracle_table(c), c.f0.copy(), "NO_WAIT", e)
    return e, commit, counts


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("name", ["CH_mod_97", "IM_ycsb3_1021_cycle"])
def test_probe_hist(name, extra):
    """A read-only epoch of exactly kProbeHistTiles * kTile accesses, and of
    one more: the probe fused with the sort's first histogram.  All txns
    commit, the digest is the oracle's, the table unchanged; then once with a
    missing key as the very last access."""
    c = I.case(name)
    n_acc = HIST_N + extra
    e, c_ref, counts = _hist_ref(name, n_acc)
    assert c_ref.all()
    eng = _engine(c, "NO_WAIT", max_txn=e.n_txn, max_acc=n_acc)
    try:
        eng.set_prefix(None)
        if extra:
            got, st = _dev_acc(eng, e)
        else:  # (the fused kernel it is: dv_kernel_times)
            out = []
            assert "k_probe_hist" in _launched(eng, lambda: out.append(_dev_acc(eng, e)))
            got, st = out[0]
        assert np.array_equal(got, c_ref) and _counts(st) == counts
        assert np.array_equal(eng.read_table(0, c.rows), c.f0)
        if extra:
            lab, k = c.missing[0]
            bad = _hist_epoch(c, n_acc, last=k)
            assert "k_probe_hist" in _launched(eng, lambda: _rejected(lambda: _dev_acc(eng, bad), what=lab))
            assert np.array_equal(eng.read_table(0, c.rows), c.f0)
    finally:
        eng.close()


# ---------------------------------------------------------------- 7. lanes over the owner's frozen tables
@pytest.mark.parametrize("name", ["CH_mod_97", "IM_mod_1021_cycle"])
def test_lanes(name):
    """Three lanes opened on the engine; eight small epochs through
    run_epochs_lanes -- epoch j reads the present keys but the last eight and
    writes the j-th of those -- each with the oracle's commit bytes, counts
    and digest, the table as `where` says.  Then, on a fresh engine, epoch 5
    holds a missing key: the call reports it and epochs 0 .. 4 are complete."""
    c = I.case(name)
    ks = c.present_keys()
    assert len(ks) > 9
    epochs = [I._mk([[(k, I.RD)] for k in ks[:-8]] + [[(ks[-1 - j], I.WR)]]) for j in range(8)]
    t, f0 = I.oracle_table(c), c.f0.copy()
    refs = []
    for e in epochs:
        commit, counts = _oracle(t, f0, "NO_WAIT", e)
        assert commit.all()
        refs.append((commit, counts, f0.copy()))
    for bad in (None, 5):
        eng = _engine(c, "NO_WAIT")
        try:
            lanes = [eng.open_lane() for _ in range(3)]
            es = list(epochs)
            if bad is not None:
                lab, k = c.missing[0]
                es[bad] = I._mk([[(x, I.RD)] for x in ks[:-8]] + [[(k, I.RD)]] + [[(ks[-1 - bad], I.WR)]])
            commits = [torch.zeros(e.n_txn, dtype=torch.uint8, device="cuda") for e in es]
            deps = [DeviceEpoch(e) for e in es]
            if bad is None:
                sts = eng.run_epochs_lanes(lanes, deps, commits)
                for j, (commit, counts, _) in enumerate(refs):
                    assert np.array_equal(commits[j].cpu().numpy(), commit) and _counts(sts[j]) == counts, j
                done = 8
            else:
                _rejected(lambda: eng.run_epochs_lanes(lanes, deps, commits), what=lab)
                for j in range(bad):
                    assert np.array_equal(commits[j].cpu().numpy(), refs[j][0]), j
                done = bad
            col = eng.read_table(0, c.rows)
            assert np.array_equal(col, refs[done - 1][2])
            assert np.array_equal(col, I.column_after(c, [ks[-1 - j] for j in range(done)]))
            # a lane decides the next epoch right
            got, st = _dev(lanes[1], epochs[done] if done < 8 else epochs[0])
            assert got[:-1].all() and np.array_equal(lanes[2].read_table(0, c.rows), eng.read_table(0, c.rows))
        finally:
            eng.close()


# ---------------------------------------------------------------- 8. the replicated branch
@pytest.mark.parametrize("world", [2, 3])
def test_replicated_probes(world):
    """Replicated epochs over dense partitions of 1,000 rows: every rank
    probes every key -- its own against its map, the others' by range.  The
    last keys of the key space commit on every rank; the first keys past it
    are DV_ERR_KEY_NOT_FOUND on every rank, whichever rank's batch holds
    them, and no partition's rows change."""
    rows, n_txn = 1000, 8
    P = world
    present = [rows * P - 1, rows * P - P]
    missing = [rows * P] + [rows * P + part for part in range(1, P)]
    engines = _engine_group(dvcc.NO_WAIT, world, rows, n_txn, mode=2)
    try:
        before = [eng.read_table(0, rows) for eng in engines]
        for p, col in enumerate(before):
            assert [int(x) for x in col[:2]] == [I.ycsb_f0(p), I.ycsb_f0(P + p)]

        def batches(key, origin):
            """rank r's batch: n_txn single reads of its own first key, `origin`'s third one reading `key`"""
            out = []
            for r in range(world):
                keys = [r] * n_txn
                if r == origin:
                    keys[2] = key
                out.append(I._mk([[(k, I.RD)] for k in keys]))
            return out
        for origin in range(world):
            for key in present:
                res = _run_group(engines, [DeviceEpoch(b) for b in batches(key, origin)], n_txn)
                for r, x in enumerate(res):
                    assert not isinstance(x, Exception), (key, origin, r, x)
                    assert x[0].all(), (key, origin, r)
            for key in missing:
                res = _run_group(engines, [DeviceEpoch(b) for b in batches(key, origin)], n_txn)
                for r, x in enumerate(res):
                    assert isinstance(x, dvcc.DvccError) and x.code == ERR_KEY, (key, origin, r, x)
                for eng, col in zip(engines, before):
                    assert np.array_equal(eng.read_table(0, rows), col), (key, origin)
        res = _run_group(engines, [DeviceEpoch(b) for b in batches(present[0], 0)], n_txn)
        assert all(not isinstance(x, Exception) and x[0].all() for x in res), res
    finally:
        for eng in engines:
            eng.close()


@pytest.mark.parametrize("world", [2, 3])
def test_replicated_probes_direct_maps(world):
    """Replicated epochs (run_epoch_part, mode 2) over partitions that are
    implicit-row direct maps but not dense (index_cases.rep_group): an own key
    is decided by direct_holds -- the home-tag bitmap where the home tag is
    the partition's own, the key-tag byte and the pkey word where it is not --
    and a foreign key by its range.  Every present key commits on every rank,
    whichever origin's batch reads it, with the digest of where[key]'s value;
    every missing one is DV_ERR_KEY_NOT_FOUND on every rank and no row
    changes; a write from a foreign origin zeroes exactly its owner's row."""
    cases = I.rep_group(world)
    n_txn = 8
    engines = []
    try:
        for p, c in enumerate(cases):
            eng = CCEngine(dvcc.NO_WAIT, n_txn * world, n_txn * world + 4096, part_cnt=world, part_id=p,
                           asynchronous=False)
            engines.append(eng)
            eng.create_table(0, c.rows, c.nbuckets, c.hash_kind)
            eng.load_table(0, np.array(c.keys, dtype=np.uint64), c.f0)
        CCEngine.comm_init_local(engines)
        for eng in engines:
            eng.comm_set_mode(2)
        safe = [c.present[0][1] for c in cases]  # what the other txns read: the rank's own first key

        def value(k):
            return int(cases[k % world].f0[k // world])

        def run(key, origin, wr=I.RD):
            bs = [I._mk([[(key, wr)] if (r == origin and j == 2) else [(safe[r], I.RD)] for j in range(n_txn)])
                  for r in range(world)]
            return dvcc.sequence(bs), _run_group(engines, [DeviceEpoch(b) for b in bs], n_txn)

        def unchanged(written, what):
            for c, eng in zip(cases, engines):
                assert np.array_equal(eng.read_table(0, c.rows), I.column_after(c, [k for k in written if k in c.where])), what
        for p, c in enumerate(cases):
            for origin in (p, (p + 1) % world):  # the owner's batch, and another rank's
                for lab, k in c.present:
                    e, res = run(k, origin)
                    digest = 0
                    for r, x in enumerate(res):
                        assert not isinstance(x, Exception), (c.name, lab, origin, r, x)
                        assert x[0].all() and x[1].committed == n_txn * world, (c.name, lab, origin, r)
                        digest = (digest + x[1].read_digest) % (1 << 64)
                    assert digest == I.read_digest([value(int(q)) for q in e.keys], e.acc_txn(), e.keys), (c.name, lab, origin)
                for lab, k in c.missing:
                    _, res = run(k, origin)
                    for r, x in enumerate(res):
                        assert isinstance(x, dvcc.DvccError) and x.code == ERR_KEY, (c.name, lab, origin, r, x)
                    unchanged([], (c.name, lab, origin))
        written = []
        for p, c in enumerate(cases):  # the last present key of each partition, written from the next rank's batch
            k = c.present[-1][1]
            _, res = run(k, (p + 1) % world, I.WR)
            assert all(not isinstance(x, Exception) and x[0].all() for x in res), (c.name, res)
            assert sum(x[1].write_cnt for x in res) == 1
            written.append(k)
            unchanged(written, (c.name, "written"))
    finally:
        for eng in engines:
            eng.close()
