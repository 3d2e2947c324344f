"""DV_SCAN accesses on the HIP engine: the substituted closed-form epochs of
tests/scan_cases.py through every path that reads a type byte.  Every epoch is
held to the formulas (scan_cases.reference: commit bytes, CALVIN's grant
groups, write count, read digest and the whole F0 column -- never the
engine's or the oracle's output), and the oracle, held to the same formulas
when the shared reference is built, is compared once more.

The engine reduces a type byte to one write bit (`== DV_WR`) wherever it reads
one, so a SCAN is a read throughout, as in the reference (row.cpp:191, :228;
ycsb_txn.cpp:228).  The readers, and the test that reaches each:
  k_probe's packed type words and its scalar tail   test_decision_paths, test_calvin_*
  row_word (a dense table's records from types)      test_prefix_kill[txn_begin]
  kk_key (the kill pass, accesses after the prefix)  test_prefix_kill[txn_begin]
  recs32 (the SCAN only in types, bit 31 clear)      test_prefix_kill[recs32]
  k_split_access / k_split_rows (host staging)       test_host_entry
  k_carry_copy, the refill's copies of types         test_carry, test_closed_loop
  the list protocol's a.type, k_split_access         test_partitioned_list
  k_group_pack_c / k_group_pack (the epoch groups)   test_partitioned_group[compact], [wide]
(profiles/scan_cases/README.md has the list with the mutations each caught.)
"""
import functools

import numpy as np
import pytest
import torch

import _oracle as O
import adversarial as A
import adversarial_calvin as AC
import dvcc
import loop_cases as LC
import scan_cases as S
from dvcc import CCEngine, DeviceEpoch, LoopTrack
from test_gpu_parity import _gpu_epoch
from test_loop_track import TrackModel
from test_loop_track_gpu import _check_track
from test_partitioned import _engine_group, _group_mine, _run_group, _run_group_epochs

pytestmark = pytest.mark.gpu

CC = {"NO_WAIT": dvcc.NO_WAIT, "WAIT_DIE": dvcc.WAIT_DIE, "OCC": dvcc.OCC, "CALVIN": dvcc.CALVIN}
OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}
U64 = 1 << 64
WITH_CALVIN = [n for n, (_, ccs) in S.FAMILIES.items() if "CALVIN" in ccs]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield
    for f in (_chain, _calvin_refs, _loop_ref, _part_refs):
        f.cache_clear()  # (the shared references go with the module)


def _oracle_held(cases, cc, rows, calls=1):
    """the epochs in sequence, `calls` times over, on one fresh table: per epoch
    the formulas' Ref, the F0 column carried by the formulas; the oracle runs
    along and is held to them.  Returns [(Ref, the oracle's digest)]."""
    tab = O.YcsbTable(rows)
    f0_or = tab.f0.copy()
    f0 = AC.initial_f0(rows)
    out = []
    for call in range(calls):
        for case in cases:
            e = case.epoch
            ref = S.reference(case, cc, f0)
            c, g, st = O.epoch_run(OCC_ID[cc], tab.ix, f0_or, e.n_txn, e.txn_begin, e.keys, e.types,
                                   want_grant=cc == "CALVIN")
            S.held(ref, c, g, st, f0_or, f"the oracle, call {call}")
            out.append((ref, st.read_digest))
            f0 = ref.f0
    return out


@functools.lru_cache(maxsize=None)
def _chain(names, patterns, cc, carried=False):
    """(cases, rows, references) of the families `names` under `patterns`, one
    after the other on one table; carried: each followed by its carried epoch,
    all of which commits"""
    cases = []
    for name, pattern in zip(names, patterns):
        case = S.substituted(name, pattern)
        cases.append(case)
        if carried:
            cases.append(A.Case(case.carried, case.rows, {cc: np.ones(case.carried.n_txn, np.uint8)}))
    rows = max(c.rows for c in cases)
    return cases, rows, _oracle_held(cases, cc, rows)


def _one(name, pattern, cc):
    cases, rows, refs = _chain((name,), (pattern,), cc)
    return cases[0], rows, refs[0]


def _engine(cc, case, rows, prefix=0, async_iters=0, **knobs):
    e = case.epoch
    eng = CCEngine(CC[cc], max(1, e.n_txn), max(1, e.n_acc), **knobs)
    eng.set_prefix(prefix)
    if async_iters:
        eng.set_async_limits(async_iters, 0)
    eng.load_ycsb_partition(rows)
    return eng


def _held(ref_or, c, g, st, table, what):
    ref, digest_or = ref_or
    S.held(ref, c, g, st, table, what)
    assert st.read_digest == digest_or, f"{what}: the oracle's read digest"


# ---- the single-GPU decision paths: k_probe's packed words and scalar tail
PATHS = {"default": {}, "sync": dict(asynchronous=False), "async": dict(async_iters=1),
         "notail_sync": dict(tail=False, asynchronous=False)}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("cc", S.DECIDING)
@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_decision_paths(name, cc, path):
    """every family under every pattern: default, synchronous rounds, the
    asynchronous launch yielding after one iteration, and rounds of
    multi-workgroup passes alone"""
    for pattern in S.PATTERNS:
        case, rows, ref = _one(name, pattern, cc)
        eng = _engine(cc, case, rows, **PATHS[path])
        try:
            c, g, st = _gpu_epoch(eng, case.epoch, "device")
            _held(ref, c, g, st, eng.read_table(0, rows), f"{name} {pattern} {cc} {path}")
        finally:
            eng.close()


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("name", WITH_CALVIN)
def test_calvin_families(name, path):
    """the same families under CALVIN: all commit, a SCAN in a run of readers
    shares their grant group and one next to a write does not"""
    for pattern in S.PATTERNS:
        case, rows, ref = _one(name, pattern, "CALVIN")
        eng = _engine("CALVIN", case, rows)
        try:
            c, g, st = _gpu_epoch(eng, case.epoch, path)
            _held(ref, c, g, st, eng.read_table(0, rows), f"{name} {pattern} CALVIN {path}")
        finally:
            eng.close()


@functools.lru_cache(maxsize=None)
def _calvin_refs(batch, pattern):
    cases, rows = S.calvin_batch(batch, pattern)
    return cases, rows, _oracle_held(cases, "CALVIN", rows)


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("batch", list(S.CALVIN_BATCHES))
def test_calvin_batches(batch, pattern, path):
    """CALVIN's own families (repeat blocks at a thread's kPV chunk and a
    kRTile tile, hidden writes, the comb, read runs and the storm), a batch's
    epochs one after the other on one engine"""
    cases, rows, refs = _calvin_refs(batch, pattern)
    eng = CCEngine(dvcc.CALVIN, max(c.epoch.n_txn for c in cases), max(c.epoch.n_acc for c in cases))
    try:
        eng.load_ycsb_partition(rows)
        for case, ref in zip(cases, refs):
            c, g, st = _gpu_epoch(eng, case.epoch, path)
            _held(ref, c, g, st, eng.read_table(0, rows), f"{case.name} {pattern} ({path})")
    finally:
        eng.close()


# ---- prefix-kill: row_word and kk_key from types, and the 4-byte records
PREFIXED = {"sweep_1": S.SWEEP_PREFIX, "sweep_63": S.SWEEP_PREFIX, "gate_odd": 256, "ladder_hot": 257,
            "carry_blocks": 300}


@pytest.mark.parametrize("form", ["txn_begin", "recs32"])
@pytest.mark.parametrize("cc", S.DECIDING)
@pytest.mark.parametrize("name", list(PREFIXED))
def test_prefix_kill(name, cc, form):
    """the epoch with its boundaries: keys and types alone (the kill pass and
    the row words read the type byte) and with 4-byte records, in which a SCAN
    is a clear bit 31 and the byte 3 stands in `types` only"""
    for pattern in S.PATTERNS:
        case, rows, ref = _one(name, pattern, cc)
        e = case.epoch
        eng = _engine(cc, case, rows, prefix=PREFIXED[name])
        try:
            dep = DeviceEpoch(e, txn_begin=True, recs32=form == "recs32")
            assert (dep.recs32 is not None) == (form == "recs32")
            if form == "recs32":
                r = dep.recs32.cpu().numpy().view(np.uint32)
                assert not (r[e.types == S.SCAN] >> 31).any() and (r[e.types == A.WR] >> 31).all()
                assert (dep.types.cpu().numpy() == S.SCAN).any()
            d = torch.zeros(e.n_txn, dtype=torch.uint8, device="cuda")
            st = eng.run_epoch_device(dep, d)
            assert st.prefix_txn == PREFIXED[name], st.prefix_txn
            _held(ref, d.cpu().numpy(), None, st, eng.read_table(0, rows), f"{name} {pattern} {cc} {form}")
        finally:
            eng.close()


# ---- the host entries: k_split_access keeps the byte, k_split_rows never sees it
@pytest.mark.parametrize("entry", ["run", "staged", "staged_rows"])
@pytest.mark.parametrize("name,cc", [("gate_odd", "NO_WAIT"), ("storm", "WAIT_DIE"), ("sweep_63", "OCC"),
                                     ("carry_ladder", "CALVIN"), ("runs_65", "CALVIN"), ("self_W", "NO_WAIT")])
def test_host_entry(name, cc, entry):
    """dv_epoch_run with dv_access.type = DV_SCAN; dv_epoch_stage_host and
    dv_epoch_stage_host_rows (the record's write bit clear), then
    dv_epoch_run_staged"""
    for pattern in S.PATTERNS:
        case, rows, ref = _one(name, pattern, cc)
        e = case.epoch
        eng = _engine(cc, case, rows)
        try:
            tb = np.ascontiguousarray(e.txn_begin, dtype=np.uint32)
            acc = e.to_access_array()
            assert (acc["type"] == dvcc.SCAN).any()
            commit = np.zeros(e.n_txn, np.uint8)
            if entry == "run":
                st = eng.run_epoch_host(acc, tb, e.n_acc, e.n_txn, commit)
            else:
                if entry == "staged":
                    eng.stage_host(0, acc, tb, e.n_acc, e.n_txn)
                else:
                    eng.stage_host_rows(0, e.to_row_records(), tb, e.n_acc, e.n_txn)
                st = eng.run_staged(0, commit)
            _held(ref, commit, None, st, eng.read_table(0, rows), f"{name} {pattern} {cc} {entry}")
        finally:
            eng.close()


# ---- carry-over: the aborted txns' SCANs travel as the byte 3
@pytest.mark.parametrize("cap_all", [True, False])
@pytest.mark.parametrize("cc", S.DECIDING)
@pytest.mark.parametrize("name", S.CARRIED)
def test_carry(name, cc, cap_all):
    """dv_epoch_carry behind the ladder with empty txns and the carry blocks,
    both with private reads: keys, types (3 exactly where the aborted txns'
    SCANs were) and txn ids against the closed form, whole and capped one
    below the carried count; then the carried epoch, all of which commits"""
    for pattern in S.PATTERNS:
        cases, rows, refs = _chain((name,), (pattern,), cc, carried=True)
        case, want = cases[0], cases[0].carried
        # (the edge pattern's SCANs are the padding txns', which commit: nothing of them is carried)
        assert (want.types == S.SCAN).any() == (pattern != "edge") and (want.types == A.WR).any()
        e = case.epoch
        cap = e.n_txn if cap_all else want.n_txn - 1
        n = min(cap, want.n_txn)
        n_acc = int(want.txn_begin[n])
        eng = _engine(cc, case, rows)
        try:
            dev = DeviceEpoch(e)
            d = torch.zeros(e.n_txn, dtype=torch.uint8, device="cuda")
            st = eng.run_epoch_device(dev, d)
            what = f"{name} {pattern} {cc}"
            _held(refs[0], d.cpu().numpy(), None, st, eng.read_table(0, rows), what)
            dc = eng.carry(dev, cap)
            assert (dc.n_txn, dc.n_acc) == (n, n_acc), what
            assert np.array_equal(dc.keys.cpu().numpy().view(np.uint64), want.keys[:n_acc]), what
            assert np.array_equal(dc.types.cpu().numpy(), want.types[:n_acc]), f"{what}: the carried types"
            assert np.array_equal(dc.acc_txn.cpu().numpy().view(np.uint32), want.acc_txn()[:n_acc]), what
            if cap_all:  # the second epoch's formula: every carried txn commits
                d2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
                st2 = eng.run_epoch_device(dc, d2)
                _held(refs[1], d2.cpu().numpy(), None, st2, eng.read_table(0, rows), f"{what}: the carried epoch")
        finally:
            eng.close()


# ---- the closed loop: the refill's copies of types
@functools.lru_cache(maxsize=None)
def _loop_ref(cc, pattern):
    """the pool, the tracker's model after LOOP_EPOCHS epochs, per epoch
    (commit formula's bytes, Ref, the oracle's stats, the host epoch), and the
    epoch the loop leaves"""
    p = S.loop_pool(pattern)
    model = TrackModel(p.P, 0, S.LOOP_N, n_bins=8)
    ref, left, f0_or = LC.run_model(CC[cc], p, model, S.LOOP_EPOCHS)  # (the oracle held to the commit formula)
    f0 = AC.initial_f0(p.rows)
    out = []
    for k, (c, st, host) in enumerate(ref):
        r, _ = S.loop_epoch_reference(p, cc, model.seen[k][0], f0)
        S.held(r, c, None, st, None, f"the oracle, epoch {k}")
        out.append((r, st.read_digest, host))
        f0 = r.f0
    assert np.array_equal(f0, f0_or)
    return p, model, out, left[S.LOOP_EPOCHS]


@pytest.mark.parametrize("form", ["types", "records"])
@pytest.mark.parametrize("cc", S.DECIDING)
def test_closed_loop(cc, form):
    """dv_epoch_run_closed_loop, four tracked epochs over loop_cases' hot-row
    pool with its reads as SCANs.  types: the keys form, the refilled epochs'
    `types` hold the byte 3 where their pool txns do.  records: the pool with
    4-byte records and a prefix of 400 txns, the tb form, whose records keep
    the write bit alone.  Commit bytes by loop_cases' formula, the commit log
    by the tracker's model, digests by the closed form."""
    pattern = "mod3" if form == "types" else "all"
    p, model, refs, nxt = _loop_ref(cc, pattern)
    n, E = S.LOOP_N, S.LOOP_EPOCHS
    eng = CCEngine(CC[cc], n, n * p.epoch.max_txn_acc())
    try:
        eng.set_prefix(None if form == "types" else 400)
        eng.load_ycsb_partition(p.rows)
        trk = LoopTrack(n, 2, log_cap=model.pos, epoch_cap=E, n_bins=8)
        trk.attach(eng)
        dpool = DeviceEpoch(p.epoch, recs32=form == "records")
        assert (dpool.recs32 is not None) == (form == "records")
        pb = torch.from_numpy(p.epoch.txn_begin.astype(np.int32)).cuda()
        commits = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop(dpool, pb, n, E, d_commits=commits, track=trk)
        assert bufs.tb == (form == "records")
        for k, (st, (ref, digest_or, host)) in enumerate(zip(sts, refs)):
            assert (st.n_txn, st.n_acc) == (host.n_txn, host.n_acc), k
            _held((ref, digest_or), commits[k].cpu().numpy(), None, st, None, f"{cc} {form}: epoch {k}")
        assert np.array_equal(eng.read_table(0, p.rows), refs[-1][0].f0)
        assert int(cursor.item()) == model.cur
        _check_track(trk, model)
        left = bufs.epoch(0, n, p.epoch.max_txn_acc())
        assert left.n_acc == nxt.n_acc
        assert np.array_equal(left.keys.cpu().numpy().view(np.uint64), nxt.keys)
        want = nxt.types if form == "types" else (nxt.types == A.WR).astype(np.uint8)
        assert (nxt.types == S.SCAN).any()
        assert np.array_equal(left.types.cpu().numpy(), want), "the refilled epoch's types"
    finally:
        eng.close()


# ---- two decision lanes
@pytest.mark.parametrize("cc", S.DECIDING)
def test_lanes(cc):
    """dv_epoch_run_device_lanes over two lanes, two consecutive substituted
    epochs on one table (the gate, then the ladder with its hot row), twice"""
    cases, rows, _ = _chain(("gate_odd", "ladder_hot"), ("mod3", "all"), cc)
    refs = _oracle_held(cases, cc, rows, calls=2)
    eng = CCEngine(CC[cc], max(c.epoch.n_txn for c in cases), max(c.epoch.n_acc for c in cases))
    try:
        eng.load_ycsb_partition(rows)
        extra = [eng.open_lane()]
        deps = [DeviceEpoch(c.epoch) for c in cases]
        commits = [torch.zeros(c.epoch.n_txn, dtype=torch.uint8, device="cuda") for c in cases]
        for call in range(2):
            sts = eng.run_epochs_lanes(extra, deps, commits)
            for k, st in enumerate(sts):
                _held(refs[2 * call + k], commits[k].cpu().numpy(), None, st, None, f"{cc}: call {call} epoch {k}")
                commits[k].zero_()
            assert np.array_equal(eng.read_table(0, rows), refs[2 * call + 1][0].f0), f"call {call}: table"
    finally:
        eng.close()


# ---- the partitioned paths, two partitions in process
WORLD = 2


@functools.lru_cache(maxsize=None)
def _part_refs(cc):
    """the partitioned ladder under `all` and under `mod3`, one after the other
    on the one-partition view of the table (row == key)"""
    base = S.part_ladder(WORLD)
    cases = [S.scan_substitute(base, pattern) for pattern in ("all", "mod3")]
    assert all(S.n_scans(c) > 0 for c in cases)
    rows_pp = -(-base.rows // WORLD)
    return cases, rows_pp, _oracle_held(cases, cc, rows_pp * WORLD)


def _sum_ranks(res, what):
    digest = writes = 0
    for r, x in enumerate(res):
        assert not isinstance(x, Exception), f"{what}: rank {r}: {x}"
        digest = (digest + x[1].read_digest) % U64
        writes += x[1].write_cnt
    return digest, writes


@pytest.mark.parametrize("cc", ["NO_WAIT", "OCC"])
def test_partitioned_list(cc):
    """dv_epoch_run_part, the list protocol: every access travels to its row's
    owner as a dv_access with its type byte.  Commit bytes on both ranks, the
    digests and write counts summed, and both partitions' rows"""
    cases, rows_pp, refs = _part_refs(cc)
    tpr = cases[0].epoch.n_txn // WORLD
    engines = _engine_group(CC[cc], WORLD, rows_pp, tpr, R=4)
    try:
        for case, (ref, digest_or) in zip(cases, refs):
            parts, tpr_ = A.contiguous_chunks(case.epoch, WORLD)
            assert tpr_ == tpr and all(p.n_txn == tpr for p in parts)
            res = _run_group(engines, [DeviceEpoch(b) for b in parts], tpr)
            digest, writes = _sum_ranks(res, cc)
            for r, (c, st) in enumerate(res):
                bad = np.flatnonzero(c != ref.commit)
                assert bad.size == 0, f"rank {r}: {bad.size} txns off the formula, first {bad[:8]}"
                assert st.committed == int(ref.commit.sum())
            assert digest == ref.digest == digest_or, "read digest"
            assert writes == ref.writes, "write count"
            for p, eng in enumerate(engines):
                assert np.array_equal(eng.read_table(0, rows_pp), ref.f0[p::WORLD]), f"partition {p} rows"
    finally:
        for eng in engines:
            eng.close()


GROUP_FORMS = ("compact", "recs32", "wide")


@pytest.mark.parametrize("form", GROUP_FORMS)
@pytest.mark.parametrize("cc", ["NO_WAIT", "OCC"])
def test_partitioned_group(cc, form):
    """dv_epoch_group_run: the two epochs as one group, each batch routed to
    the epoch's decider and from there to the owners.  compact: 4-byte words
    (row | start << 30 | write << 31) packed from keys and types; recs32: the
    same words from the batches' 4-byte records, the SCAN in `types` alone;
    wide: 8 bytes an access (DV_COMM_WIDE_BATCHES), packed from keys and types"""
    cases, rows_pp, refs = _part_refs(cc)
    tpr = cases[0].epoch.n_txn // WORLD
    engines = _engine_group(CC[cc], WORLD, rows_pp, tpr, R=4,
                            mode=2 | (dvcc._lib.DV_COMM_WIDE_BATCHES if form == "wide" else 0))
    try:
        parts = [A.cut(case.epoch, WORLD, "origin")[0] for case in cases]
        homes = [[DeviceEpoch(parts[e][r], recs32=form == "recs32") for e in range(WORLD)] for r in range(WORLD)]
        assert all((h.recs32 is not None) == (form == "recs32") and (h.types == S.SCAN).any() for hs in homes for h in hs)
        res = _run_group_epochs(engines, homes, tpr)
        digest, writes = _sum_ranks(res, cc)
        for r, (c, st) in enumerate(res):
            for e, (ref, _) in enumerate(refs):
                mine = _group_mine(ref.commit, r, tpr, WORLD, CC[cc], False)
                got = c[e * tpr:(e + 1) * tpr]
                assert np.array_equal(got, mine), f"epoch {e} rank {r}: {int((got != mine).sum())} txns off the formula"
            assert st.committed == sum(int(ref.commit.sum()) for ref, _ in refs)
        assert digest == sum(ref.digest for ref, _ in refs) % U64 == sum(d for _, d in refs) % U64, "read digest"
        assert writes == sum(ref.writes for ref, _ in refs), "write count"
        for p, eng in enumerate(engines):
            assert np.array_equal(eng.read_table(0, rows_pp), refs[-1][0].f0[p::WORLD]), f"partition {p} rows"
    finally:
        for eng in engines:
            eng.close()
