"""The closed-form adversarial epochs of tests/adversarial.py on the HIP
engine: every case bit for bit against `expected_commit` (a formula, never the
oracle's or the engine's output) AND against the CPU oracle -- commit bytes,
committed / aborted / write counts, the read digest, CALVIN's grant groups and
the whole F0 column after each epoch.

What the families reach that a zipf workload does not: dependency chains
thousands deep (k_round_tail's loop, k_round_async's iterations and its
yield-and-resume, run_rounds' rounds queued past the fixpoint, the round log
past its 64 entries), a queue that stays undecided across many slices of the
asynchronous launch, runs at the wave / block / tile / workgroup-capacity
boundaries, the tail capacities, the top bits of a 32-bit round element and
the switch to 64-bit ones, every row of the prefix kill's bitmap, hot-row copy
and Bloom filter, and carry-over of empty, all-carried and nothing-carried
blocks.
"""
import functools

import numpy as np
import pytest
import torch

import _oracle as O
import adversarial as A
import dvcc
from dvcc import CCEngine, DeviceEpoch
from test_carry import _check_loop
from test_gpu_parity import _gpu_epoch
from test_partitioned import _engine_group, _oracle_global, _run_group

pytestmark = pytest.mark.gpu

CC = {"NO_WAIT": dvcc.NO_WAIT, "WAIT_DIE": dvcc.WAIT_DIE, "OCC": dvcc.OCC, "CALVIN": dvcc.CALVIN}
OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC, "CALVIN": O.CALVIN}
DECIDING = ("NO_WAIT", "WAIT_DIE", "OCC")
K = A.structural_constants()

LADDER_L = 3001


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield
    for f in (_built, _ref, _sweep, _sweep_refs, _width, _width_ref, _carry_case):
        f.cache_clear()  # (the shared references go with the module)


def _small_cases():
    cs = {"ladder": lambda: A.ladder(LADDER_L),
          # hot queue 6 of every 8 accesses (75 %): more than 128 slices of a whole
          # chip's asynchronous launch, more than 32 of a quarter-chip lane's
          # (OCC: about L rounds; NO_WAIT / WAIT_DIE settle it in about 10, see ladder_gate)
          "ladder_hot": lambda: A.ladder_hot(LADDER_L, 5),
          # the hot queue 2 of every 3 accesses, undecided for L rounds under every
          # algorithm; the gate commits (L odd) and aborts (L even)
          "gate_odd": lambda: A.ladder_gate(LADDER_L, 4 * LADDER_L),
          "gate_even": lambda: A.ladder_gate(LADDER_L - 1, 4 * LADDER_L),
          "self_R": lambda: A.self_conflict(A.RD), "self_W": lambda: A.self_conflict(A.WR)}
    # family 3: m = B - 1, B, B + 1 readers per run.  B is a size of the kernels'
    # geometry, as the issue lists them; what a run of m equal requests on one row
    # straddles is the structure of that size in whichever kernel holds the whole
    # queue (a wave's or a block's scan, a tile of the pass).  An asynchronous
    # workgroup's slice is n_all / G elements -- a few hundred here -- so m = kAsyncCap
    # +- 1 is NOT a slice edge of k_round_async; it is the size past which one
    # workgroup could no longer hold the run.
    for what, B in (("wave", 64),                        # a wave
                    ("kBlock", K["kBlock"]),             # 256 (csrc/dvcc_internal.h)
                    ("kAsyncThreads", K["kAsyncThreads"]),  # 1,024 (csrc/dvcc_rounds.hip)
                    # round 0's tile of sorted pairs and a pass over 64-bit elements:
                    # DVCC_ROUND_T64 1,024 threads x DVCC_ROUND_IPT64 4 = 4,096 (csrc/dvcc_rounds.hip, Geo)
                    ("kTile64", K["kTile64"]),
                    # the synchronous pass's tile of 32-bit elements: 1,024 threads x
                    # DVCC_ROUND_IPT 16 = 16,384 (csrc/dvcc_rounds.hip, Geo)
                    ("kTile", K["kTile"]),
                    # kAsyncCap, the most elements one asynchronous workgroup takes:
                    # kAsyncThreads 1,024 x DVCC_ASYNC_IPT 28 = 28,672 (csrc/dvcc_rounds.hip)
                    ("kAsyncCap", K["kAsyncCap"])):
        for d in (-1, 0, 1):
            cs[f"runs_{what}{d:+d}"] = functools.partial(A.read_runs, B + d)
    # family 4: the tail's capacities, TailGeo::kCap = kTailThreads 1,024 x 16 = 16,384
    # 32-bit elements / x 12 = 12,288 64-bit ones (csrc/dvcc_rounds.hip), +- 1; and 40,000
    for n in (K["kTailCap64"] - 1, K["kTailCap64"] + 1, K["kTailCap32"] - 1, K["kTailCap32"] + 1, 40_000):
        cs[f"storm_{n}"] = functools.partial(A.writer_storm, n)
    return cs


SMALL = _small_cases()


# family 3 has r = 5 runs; under WAIT_DIE alone fewer at the two largest B, where the
# ORACLE walks the row's committed readers for every request (33 s at m = 28,673,
# r = 5): 3 and 2 runs still hold a first run, a writer, and a run and a writer
# behind a writer
RUNS_R_WAIT_DIE = {"kTile": 3, "kAsyncCap": 2}


@functools.lru_cache(maxsize=None)
def _built(name, r):
    return SMALL[name](r) if r else SMALL[name]()


def _case(name, cc=None):
    if not name.startswith("runs_"):
        return _built(name, 0)
    what = name[5:-2]
    return _built(name, RUNS_R_WAIT_DIE.get(what, 5) if cc == "WAIT_DIE" else 5)


def _oracle_runs(case, cc, times=1):
    """the oracle over `case`'s epoch `times` times on one table: per run
    (commit, grant, counts, F0 after it)"""
    tab = O.YcsbTable(case.rows)
    f0 = tab.f0.copy()
    e = case.epoch
    out = []
    for _ in range(times):
        c, g, st = O.epoch_run(OCC_ID[cc], tab.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types,
                               want_grant=cc == "CALVIN")
        out.append((c.copy(), g, (st.committed, st.aborted, st.write_cnt, st.read_digest), f0.copy()))
    return out


@functools.lru_cache(maxsize=None)
def _ref(name, cc):
    return _oracle_runs(_case(name, cc), cc)[0]


def _same(case, cc, ref, c, g, st, table, what=""):
    """one epoch's outcome against the formula and the oracle"""
    c_ref, g_ref, counts, f0 = ref
    exp = case.expected_commit(cc)
    assert np.array_equal(c, exp), f"{what}: {int((c != exp).sum())} txns off the formula, first {np.flatnonzero(c != exp)[:8]}"
    assert np.array_equal(c, c_ref), f"{what}: {int((c != c_ref).sum())} txns off the oracle"
    if cc == "CALVIN":
        assert np.array_equal(g, g_ref), f"{what}: grant mismatch: {int((g != g_ref).sum())}"
        if case.grant is not None:
            assert np.array_equal(g, case.grant), f"{what}: grants off the formula"
    assert (st.committed, st.aborted, st.write_cnt, st.read_digest) == counts, what
    assert st.committed == int(exp.sum()) and st.aborted == int((1 - exp).sum()), what
    assert np.array_equal(table, f0), f"{what}: table state mismatch"


def _run(case, cc, ref, prefix=0, async_iters=0, **knobs):
    e = case.epoch
    eng = CCEngine(CC[cc], max(1, e.n_txn), max(1, e.n_acc), **knobs)
    try:
        eng.set_prefix(prefix)
        if async_iters:
            eng.set_async_limits(async_iters, 0)
        eng.load_ycsb_partition(case.rows)
        c, g, st = _gpu_epoch(eng, e, "device")
        _same(case, cc, ref, c, g, st, eng.read_table(0, case.rows))
    finally:
        eng.close()
    return st


# ---- families 1-5 on every decision path
PATHS = {"default": {}, "sync": dict(asynchronous=False), "notail_sync": dict(tail=False, asynchronous=False),
         "el64": dict(el64=True), "iters1": dict(async_iters=1), "iters3": dict(async_iters=3),
         "lsd": dict(lsd_sort=True),
         # the cut on a committing (256) and on an aborting (257) ladder txn
         "prefix256": dict(prefix=256), "prefix257": dict(prefix=257)}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("cc", DECIDING)
@pytest.mark.parametrize("name", list(SMALL))
def test_families_1_to_5(name, cc, path):
    st = _run(_case(name, cc), cc, _ref(name, cc), **PATHS[path])
    if name in ("ladder", "gate_odd", "gate_even") and path == "notail_sync":
        # every round is one multi-workgroup pass, which cannot decide a chain
        # link in less than a pass; loose on purpose (a pass may see a status
        # stored earlier in the same pass).  Measured: one round per link.
        assert st.rounds >= (LADDER_L - 1) // 4, st.rounds
    if name in ("ladder", "gate_odd", "gate_even") and path in ("iters1", "iters3"):
        assert st.async_launches and st.async_yields, "the asynchronous launch was to yield mid-chain"
    if path.startswith("prefix") and _case(name, cc).epoch.n_txn > 257:
        assert st.prefix_txn == PATHS[path]["prefix"]


@pytest.mark.parametrize("name", list(SMALL))
def test_families_1_to_5_calvin(name):
    _run(_case(name, "CALVIN"), "CALVIN", _ref(name, "CALVIN"))


GRAPH_CALLS = 6


@pytest.mark.parametrize("cc", DECIDING)
def test_families_lanes_graph_replayed(cc):
    """dv_epoch_run_device_lanes over four quarter-chip lanes, GRAPH_CALLS
    calls of the same eight epochs from the same DeviceEpochs into the same
    commit buffers (zeroed in between), so every (lane, buffers, commit
    pointer) key comes once per call on the same lane: graph_decide
    (csrc/dvcc_runtime.hip, kGraphAfter = 3) runs it plainly twice, captures
    its decision and execution at the third call and replays the graph at
    calls 4 to 6.  Every call is read back and checked against the formula
    and the oracle, and the table after it.  The chains yield in the
    asynchronous launch (the lanes then run the halted epoch again), so the
    replays cover the host walk with launches skipped, the replayed yield and
    the halt; family 2's and the gates' hot queues span a quarter-chip lane's
    slices.  Lane k % 4 takes epoch k: ladder and self_W on lane 0,
    ladder_hot and read runs on 1, gate_even and gate_odd on 2, the storm and
    self_R on 3."""
    names = ["ladder", "ladder_hot", "gate_even", f"storm_{K['kTailCap32'] + 1}",
             "self_W", "runs_kBlock+1", "gate_odd", "self_R"]
    cases = [_case(n, cc) for n in names]
    rows = max(c.rows for c in cases)
    tab = O.YcsbTable(rows)
    f0 = tab.f0.copy()
    eng = CCEngine(CC[cc], max(c.epoch.n_txn for c in cases), max(c.epoch.n_acc for c in cases))
    try:
        eng.load_ycsb_partition(rows)
        eng.set_prefix(None)
        extra = [eng.open_lane() for _ in range(3)]
        deps = [DeviceEpoch(c.epoch) for c in cases]
        commits = [torch.zeros(c.epoch.n_txn, dtype=torch.uint8, device="cuda") for c in cases]
        yields = 0
        for call in range(GRAPH_CALLS):
            sts = eng.run_epochs_lanes(extra, deps, commits)
            for k, (case, st) in enumerate(zip(cases, sts)):
                e = case.epoch
                c_ref, _, st_ref = O.epoch_run(OCC_ID[cc], tab.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types)
                what = f"call {call} epoch {k} ({names[k]})"
                c = commits[k].cpu().numpy()
                exp = case.expected_commit(cc)
                assert np.array_equal(c, exp), f"{what}: {int((c != exp).sum())} txns off the formula"
                assert np.array_equal(c, c_ref), what
                assert (st.committed, st.aborted, st.write_cnt, st.read_digest) == (
                    st_ref.committed, st_ref.aborted, st_ref.write_cnt, st_ref.read_digest), what
                if call >= 3:
                    yields += st.async_yields
                commits[k].zero_()  # (the next call has to write every byte again)
            assert np.array_equal(eng.read_table(0, rows), f0), f"call {call}: table state mismatch"
        assert yields > 0, "no replayed epoch yielded in its asynchronous launch"
    finally:
        eng.close()


# ---- family 6: every row against the prefix kill's three structures
SWEEP_ROWS, SWEEP_P = (1 << 21) + 37, 4096


# (cc is the slowest parameter, the prefix the fastest: consecutive tests share a
# reference; about 30 MB a case and 70 MB a reference, so the caches stay small)
@functools.lru_cache(maxsize=4)
def _sweep(sweep_wr, acc_mod):
    return A.row_sweep(SWEEP_ROWS, SWEEP_P, sweep_wr, acc_mod)


@functools.lru_cache(maxsize=1)
def _sweep_refs(cc, sweep_wr, acc_mod):
    return _oracle_runs(_sweep(sweep_wr, acc_mod), cc, times=3)


@pytest.mark.parametrize("prefix", [SWEEP_P, 0])
@pytest.mark.parametrize("acc_mod", [1, 63])
@pytest.mark.parametrize("sweep_wr", [0, 1])
@pytest.mark.parametrize("cc", DECIDING)
def test_row_sweep(cc, sweep_wr, acc_mod, prefix):
    """kHotRows = 65,536 rows in the LDS copy, a 2^20-bit Bloom filter for the
    rest (csrc/dvcc_prefix.hip): 2^21 + 37 rows put two rows on every Bloom
    bit and leave the bitmap's last word with 5 rows.  The epoch through both
    range sources (its own boundaries, with 4-byte records or keys and types,
    and acc_txn), one after the other on one table; the prefix the caller's
    4,096 txns and the automatic cut."""
    case = _sweep(sweep_wr, acc_mod)
    assert case.extra["prefix_acc"] % 64 == acc_mod
    refs = _sweep_refs(cc, sweep_wr, acc_mod)
    e = case.epoch
    eng = CCEngine(CC[cc], e.n_txn, e.n_acc)
    try:
        eng.load_ycsb_partition(case.rows)
        eng.set_prefix(prefix)
        for k, (with_tb, recs) in enumerate(((True, True), (True, False), (False, False))):
            dep = DeviceEpoch(e, txn_begin=with_tb, recs32=recs)
            assert (dep.recs32 is not None) == recs
            d = torch.zeros(e.n_txn, dtype=torch.uint8, device="cuda")
            st = eng.run_epoch_device(dep, d)
            assert st.prefix_txn == SWEEP_P if prefix else st.prefix_txn > 0, st.prefix_txn
            _same(case, cc, refs[k], d.cpu().numpy(), None, st, eng.read_table(0, case.rows),
                  what=f"txn_begin={with_tb} recs32={recs}")
    finally:
        eng.close()


# ---- family 7: the top bits of a 32-bit round element, and one txn more
@functools.lru_cache(maxsize=1)
def _width(n_txn):
    return A.width_boundary(n_txn)


@functools.lru_cache(maxsize=1)
def _width_ref(n_txn, cc):
    return _oracle_runs(_width(n_txn), cc)[0]


@pytest.mark.parametrize("path", ["default", "sync", "notail_sync"])
@pytest.mark.parametrize("cc", ["NO_WAIT", "OCC"])
@pytest.mark.parametrize("n_txn", [1 << 22, (1 << 22) + 1])
def test_element_width_boundary(n_txn, cc, path):
    """slog = 7 (a 128-access txn): 2^22 txns are the most round_el32() packs
    into 32 bits -- the ladder at the highest txn ids sets bits 27..31 -- and
    2^22 + 1 switch the epoch to 64-bit elements.  Prefix kill off: its
    stages renumber into small sub-epochs and never set the top bits.  (No
    field of dv_stats reports the element width, so the switch itself is
    asserted only through round_el32's rule above.)"""
    _run(_width(n_txn), cc, _width_ref(n_txn, cc), prefix=None, **PATHS[path])


# ---- family 8: carry-over of irregular txns
@functools.lru_cache(maxsize=None)
def _carry_case(which):
    # kCarryTpb = kBlock = 256 txns per block of k_carry_copy (csrc/dvcc_carry.hip)
    return A.ladder(1001, empties=True) if which == "ladder" else A.carry_blocks(K["kBlock"])


@pytest.mark.parametrize("cap_all", [True, False])
@pytest.mark.parametrize("which", ["ladder", "blocks"])
@pytest.mark.parametrize("cc", DECIDING)
def test_carry_closed_form(cc, which, cap_all):
    """eng.carry of an epoch with empty txns between the carried ones (and of
    whole blocks of empty, carried and kept txns): keys, types and txn ids
    against the closed form, capped at N and one below the carried count;
    then the carried epoch itself, all of which commits"""
    case = _carry_case(which)
    e, want = case.epoch, case.carried
    cap = e.n_txn if cap_all else want.n_txn - 1
    n = min(cap, want.n_txn)
    tab = O.YcsbTable(case.rows)
    f0 = tab.f0.copy()
    c_ref, _, st_ref = O.epoch_run(OCC_ID[cc], tab.ix, f0, e.n_txn, e.txn_begin, e.keys, e.types)
    eng = CCEngine(CC[cc], e.n_txn, max(1, e.n_acc))
    try:
        eng.load_ycsb_partition(case.rows)
        dev = DeviceEpoch(e)
        d = torch.zeros(e.n_txn, dtype=torch.uint8, device="cuda")
        st = eng.run_epoch_device(dev, d)
        _same(case, cc, (c_ref, None, (st_ref.committed, st_ref.aborted, st_ref.write_cnt, st_ref.read_digest), f0),
              d.cpu().numpy(), None, st, eng.read_table(0, case.rows))
        dc = eng.carry(dev, cap)
        n_acc = int(want.txn_begin[n])
        assert (dc.n_txn, dc.n_acc) == (n, n_acc)
        assert np.array_equal(dc.keys.cpu().numpy().view(np.uint64), want.keys[:n_acc])
        assert np.array_equal(dc.types.cpu().numpy(), want.types[:n_acc])
        assert np.array_equal(dc.acc_txn.cpu().numpy().view(np.uint32), want.acc_txn()[:n_acc])
        # the carried epoch, run next
        c2_ref, _, st2_ref = O.epoch_run(OCC_ID[cc], tab.ix, f0, n, want.txn_begin[:n + 1].copy(),
                                         want.keys[:n_acc].copy(), want.types[:n_acc].copy())
        d2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st2 = eng.run_epoch_device(dc, d2)
        c2 = d2.cpu().numpy()
        assert c2.all() and np.array_equal(c2, c2_ref)
        assert (st2.committed, st2.aborted, st2.write_cnt, st2.read_digest) == (n, 0, st2_ref.write_cnt,
                                                                               st2_ref.read_digest)
        assert np.array_equal(eng.read_table(0, case.rows), f0)
    finally:
        eng.close()


@pytest.mark.parametrize("which", ["ladder", "blocks"])
@pytest.mark.parametrize("cc", DECIDING)
def test_carry_closed_loop(cc, which):
    """the same txns as the pool of dv_epoch_run_closed_loop, 3 epochs against
    the oracle's host loop: commit bytes, counts, digests, the epoch the loop
    leaves, the cursor and the table"""
    case = _carry_case(which)
    pool = case.epoch
    n_txn = 700 if which == "ladder" else 600
    eng = CCEngine(CC[cc], n_txn, n_txn * pool.max_txn_acc())
    try:
        eng.load_ycsb_partition(case.rows)
        _check_loop(eng, CC[cc], case.rows, pool, n_txn, 3)
    finally:
        eng.close()


# ---- one partitioned case
@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("cc", ["NO_WAIT", "OCC"])
def test_partitioned_ladder(cc, world):
    """Ladder(301) cut into contiguous chunks across in-process partitions,
    origin-major.  Key k lives on partition k % world, so every txn spans two
    partitions and every link of the chain costs a vote.  Expected commits:
    the formula in global sequence order (the last chunk's unused slots are
    empty txns, which commit)."""
    case = A.ladder(301)
    parts, tpr = A.contiguous_chunks(case.epoch, world)
    rows_pp = 512 // world
    padded = [dvcc.Epoch(b.keys, b.types, np.concatenate([b.txn_begin, np.full(tpr - b.n_txn, b.txn_begin[-1],
                                                                                np.uint32)])) for b in parts]
    c_ref, st_ref, f0 = _oracle_global(CC[cc], padded, world, rows_pp)
    exp = np.ones(tpr * world, np.uint8)
    exp[:301] = case.expected_commit(cc)
    assert np.array_equal(c_ref, exp)
    engines = _engine_group(CC[cc], world, rows_pp, tpr, R=2)
    try:
        res = _run_group(engines, [DeviceEpoch(b) for b in parts], tpr)
        digest = writes = 0
        for r, x in enumerate(res):
            assert not isinstance(x, Exception), f"rank {r}: {x}"
            c, st = x
            assert np.array_equal(c, exp), f"rank {r}: {int((c != exp).sum())} txns off the formula"
            assert st.committed == st_ref.committed == int(exp.sum())
            digest = (digest + st.read_digest) % (1 << 64)
            writes += st.write_cnt
        assert digest == st_ref.read_digest and writes == st_ref.write_cnt
        for p, eng in enumerate(engines):
            assert np.array_equal(eng.read_table(0, rows_pp), f0[p::world]), f"partition {p} table"
    finally:
        for eng in engines:
            eng.close()
