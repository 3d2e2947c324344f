"""The closed-form CALVIN epochs of tests/adversarial_calvin.py on the HIP
engine.  Every comparison is exact equality, against the formula (never the
engine's own output) and against the CPU oracle, which the shared reference
holds to the formula first: commit bytes, grant groups, committed / aborted,
write count, read digest and the whole F0 column after every epoch.

What the families reach that zipf and random epochs are unlikely to draw:
  repeat blocks  a txn's repeat run on one row across a thread's kPV chunk, a
                 wave's and a workgroup's chunk of k_seg_prepare (EL_DUP, the
                 pairs[i - 2] look-behind, prev_entry_wr) and across a thread's
                 kRIPT entries and a kRTile tile of k_calvin_pass;
                 k_calvin_dup_fix over runs of 2, 3 and kMaxPos - 4
  hidden write   a queue whose boundary count stays 0 while its seen-a-write
                 bit travels through the look-back of several tiles
  comb           queue heads at every alignment, all eight short queues,
                 k_exec's scalar tail at every access count mod kPV, sequence
                 order against row order

Cases are batched: one engine runs a batch's epochs in sequence, each case on
hot rows of its own, the F0 column carried by the formula.  The paths: one
context (host epoch, DeviceEpoch, the lsd_sort knob, which CALVIN accepts),
four decision lanes with graph replay, and the partitioned paths in process
(list protocol, replicated, epoch-group route: walk_row_queues' RT_SEESW) at
world 2 and 3.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import _oracle as O
import adversarial as A
import adversarial_calvin as AC
import dvcc
from adversarial_calvin import K
from dvcc import CCEngine, DeviceEpoch
from test_gpu_parity import _gpu_epoch
from test_partitioned import _engine_group, _run_group, _run_group_epochs

pytestmark = pytest.mark.gpu

U64 = 1 << 64
GRAPH_CALLS = 6
Ref = namedtuple("Ref", "digest writes f0")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield
    for f in (_batch, _refs, _part):
        f.cache_clear()  # (the shared references go with the module)


def _hidden(x0=1):
    return [AC.hidden_write(m, x0 + i) for i, m in enumerate(AC.hidden_write_sizes())]


BATCHES = {f"repeat_{what}": functools.partial(AC.repeat_blocks, B) for what, B in AC.REPEAT_B.items()}
BATCHES["hidden"] = _hidden
BATCHES["comb"] = AC.comb_epochs
# families 3 and 4 with their values: runs of kRTile + 1 readers (run 0 sees the
# initial value, later runs 0 through the look-back), then the storm, whose
# private reads see the initial value (it only writes row 0, which the runs wrote)
BATCHES["runs_storm"] = lambda: [AC.read_runs(K["kRTile"] + 1, 3), AC.writer_storm(K["kRTile"] + 1)]
# the partitioned paths' six epochs: the hidden writes and the comb in both orders
_COMB_R = 2 * K["kRTile"] + 37
BATCHES["part"] = lambda: _hidden() + [AC.comb(_COMB_R, 4, shift=5),
                                       AC.comb(_COMB_R, 4 + _COMB_R + 1, shift=6, reverse=True)]


@functools.lru_cache(maxsize=None)
def _batch(name):
    return BATCHES[name]()


def _reference(cases, rows, calls):
    """The batch's epochs in sequence, `calls` times over, on one table: per
    epoch the formula's (digest, write count, F0 after), the F0 column carried
    by the formula; the oracle runs along and is held to it."""
    tab = O.YcsbTable(rows)
    f0_or = tab.f0.copy()
    f0 = AC.initial_f0(rows)
    out = []
    for call in range(calls):
        for case in cases:
            e = case.epoch
            digest, writes, f0 = AC.outcome(case, f0)
            c, g, st = O.epoch_run(O.CALVIN, tab.ix, f0_or, e.n_txn, e.txn_begin, e.keys, e.types, want_grant=True)
            assert c.all() and np.array_equal(g, case.grant), f"{case.name}: the oracle off the formula"
            assert (st.committed, st.aborted, st.write_cnt, st.read_digest) == (e.n_txn, 0, writes, digest), case.name
            assert np.array_equal(f0, f0_or), case.name
            out.append(Ref(digest, writes, f0))
    return out


@functools.lru_cache(maxsize=None)
def _refs(name):
    """GRAPH_CALLS calls' worth, computed once: a single pass over the batch
    uses the first len(cases) of them"""
    cases = _batch(name)
    return _reference(cases, max(c.rows for c in cases), GRAPH_CALLS)


def _same(case, ref, c, g, st, table, what):
    assert len(c) == case.epoch.n_txn and c.all(), f"{what}: {int((c == 0).sum())} txns not committed"
    if g is not None:
        bad = np.flatnonzero(g != case.grant)
        assert bad.size == 0, f"{what}: {bad.size} grants off the formula, first at accesses {bad[:8]}"
    assert (st.committed, st.aborted) == (case.epoch.n_txn, 0), what
    assert st.write_cnt == ref.writes, f"{what}: write count"
    assert st.read_digest == ref.digest, f"{what}: read digest"
    if table is not None:
        bad = np.flatnonzero(table != ref.f0)
        assert bad.size == 0, f"{what}: {bad.size} rows off the formula, first {bad[:8]}"


# ---- one context
@pytest.mark.parametrize("path", ["host", "device", "lsd"])
@pytest.mark.parametrize("name", [n for n in BATCHES if n != "part"])
def test_one_context(name, path):
    """a batch's epochs one after the other on one engine: from host buffers,
    from DeviceEpochs, and with lsd_sort=True (the plain LSD passes)"""
    cases, refs = _batch(name), _refs(name)
    rows = max(c.rows for c in cases)
    eng = CCEngine(dvcc.CALVIN, max(c.epoch.n_txn for c in cases), max(c.epoch.n_acc for c in cases),
                   lsd_sort=path == "lsd")
    try:
        eng.load_ycsb_partition(rows)
        for case, ref in zip(cases, refs):
            c, g, st = _gpu_epoch(eng, case.epoch, "host" if path == "host" else "device")
            _same(case, ref, c, g, st, eng.read_table(0, rows), f"{case.name} ({path})")
    finally:
        eng.close()


# ---- four decision lanes, graph replay
@pytest.mark.parametrize("name", [n for n in BATCHES if n != "part"])
def test_lanes_graph_replayed(name):
    """dv_epoch_run_device_lanes over four lanes, GRAPH_CALLS calls of the
    batch's epochs from the same DeviceEpochs into the same commit buffers
    (zeroed in between): plain runs, the capture at the third call, replays
    after it (graph_decide, kGraphAfter = 3; the look-back descriptors are
    cleared inside the replayed epoch).  From call 2 on every read of a row
    the batch writes sees 0; the F0 column is the formula's throughout."""
    cases, refs = _batch(name), _refs(name)
    rows = max(c.rows for c in cases)
    eng = CCEngine(dvcc.CALVIN, max(c.epoch.n_txn for c in cases), max(c.epoch.n_acc for c in cases))
    try:
        eng.load_ycsb_partition(rows)
        extra = [eng.open_lane() for _ in range(3)]
        deps = [DeviceEpoch(c.epoch) for c in cases]
        commits = [torch.zeros(c.epoch.n_txn, dtype=torch.uint8, device="cuda") for c in cases]
        for call in range(GRAPH_CALLS):
            sts = eng.run_epochs_lanes(extra, deps, commits)
            for k, (case, st) in enumerate(zip(cases, sts)):
                _same(case, refs[call * len(cases) + k], commits[k].cpu().numpy(), None, st, None,
                      f"call {call} epoch {k} ({case.name})")
                commits[k].zero_()  # (the next call has to write every byte again)
            bad = np.flatnonzero(eng.read_table(0, rows) != refs[(call + 1) * len(cases) - 1].f0)
            assert bad.size == 0, f"call {call}: {bad.size} rows off the formula, first {bad[:8]}"
    finally:
        eng.close()


# ---- the partitioned paths, in process
@functools.lru_cache(maxsize=None)
def _part(world):
    """the partitioned batch with every epoch padded with empty txns to
    txns_per_rank * world txns (so the contiguous cut keeps the epoch's txn
    ids), its reference on the one-partition view (row == key), and per epoch
    the origins' batches"""
    cases = _batch("part")
    tpr = -(-max(c.epoch.n_txn for c in cases) // world)
    cases = [AC.padded(c, tpr * world) for c in cases]
    rows_pp = -(-max(c.rows for c in cases) // world)
    refs = _reference(cases, rows_pp * world, 1)
    f0 = AC.initial_f0(rows_pp * world)
    for case, ref in zip(cases, refs):
        # the case cannot degenerate: a read that has to carry "sees an earlier
        # write" (RT_SEESW on the route) on a row that held a non-zero value
        rows = case.epoch.keys.astype(np.int64)
        assert (case.sees0 & (f0[rows] != 0)).any(), case.name
        f0 = ref.f0
    parts = []
    for case in cases:
        ps, tpr_ = A.cut(case.epoch, world, "origin")
        assert tpr_ == tpr and sum(p.n_acc for p in ps) == case.epoch.n_acc
        parts.append(ps)
    return cases, refs, parts, tpr, rows_pp


def _sum_ranks(res, what):
    digest = writes = 0
    for r, x in enumerate(res):
        assert not isinstance(x, Exception), f"{what}: rank {r}: {x}"
        digest = (digest + x[1].read_digest) % U64
        writes += x[1].write_cnt
    return digest, writes


def _check_rows(engines, ref, world, rows_pp, what):
    for p, eng in enumerate(engines):
        bad = np.flatnonzero(eng.read_table(0, rows_pp) != ref.f0[p::world])
        assert bad.size == 0, f"{what}: partition {p}: {bad.size} rows off the formula, first {bad[:8]}"


@pytest.mark.parametrize("mode", ["list", "replicated"])
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_epochs(world, mode):
    """dv_epoch_run_part, one epoch per call on one engine group: the list
    protocol (every owner queues the records it receives; the hidden write's
    queue lands whole on one owner) and the replicated mode (every rank queues
    the whole epoch and executes its own rows).  Row r lives on partition
    r % world as local row r / world, off a power of two at world 3."""
    cases, refs, parts, tpr, rows_pp = _part(world)
    engines = _engine_group(dvcc.CALVIN, world, rows_pp, tpr, mode=1 if mode == "list" else 2)
    try:
        for case, ref, ps in zip(cases, refs, parts):
            what = f"{case.name} ({mode}, world {world})"
            res = _run_group(engines, [DeviceEpoch(p) for p in ps], tpr)
            digest, writes = _sum_ranks(res, what)
            for r, (c, st) in enumerate(res):
                assert len(c) == tpr * world and c.all(), f"{what}: rank {r}: {int((c == 0).sum())} txns not committed"
                assert (st.committed, st.aborted) == (tpr * world, 0), f"{what}: rank {r}"
            assert digest == ref.digest, f"{what}: read digest"
            assert writes == ref.writes, f"{what}: write count"
            _check_rows(engines, ref, world, rows_pp, what)
    finally:
        for eng in engines:
            eng.close()


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_group_route(world):
    """dv_epoch_group_run: `world` epochs per group, epoch e queued by rank e
    alone, whose walk_row_queues hands every read behind an earlier txn's
    write to its owner with RT_SEESW; the owners execute in epoch order."""
    cases, refs, parts, tpr, rows_pp = _part(world)
    assert len(cases) % world == 0
    engines = _engine_group(dvcc.CALVIN, world, rows_pp, tpr, mode=2)
    try:
        for g0 in range(0, len(cases), world):
            what = f"group {g0 // world} (world {world}: {', '.join(c.name for c in cases[g0:g0 + world])})"
            homes = [[DeviceEpoch(parts[g0 + e][r]) for e in range(world)] for r in range(world)]
            res = _run_group_epochs(engines, homes, tpr)
            digest, writes = _sum_ranks(res, what)
            for r, (c, st) in enumerate(res):
                assert len(c) == tpr * world and c.all(), f"{what}: rank {r}: {int((c == 0).sum())} txns not committed"
                assert (st.committed, st.aborted) == (tpr * world * world, 0), f"{what}: rank {r}"
                assert st.n_txn == tpr * world * world
            group = refs[g0:g0 + world]
            assert digest == sum(x.digest for x in group) % U64, f"{what}: read digest"
            assert writes == sum(x.writes for x in group), f"{what}: write count"
            _check_rows(engines, group[-1], world, rows_pp, what)
    finally:
        for eng in engines:
            eng.close()
