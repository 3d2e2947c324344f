"""DV_SCAN accesses in the closed-form epochs (a plain module, shared by
test_scan_cases_cpu.py and test_scan_cases_gpu.py).

The rule.  In the reference a SCAN is a shared access that reads the row:
storage/row.cpp:191 and :228 take LOCK_SH for `RD || SCAN`, row.cpp:257 hands
the row out, and benchmarks/ycsb_txn.cpp:228 reads the field for `acctype ==
RD || acctype == SCAN`.  Nothing else tells the two apart (range scans,
SCAN_LEN, are no part of the engine).  So an epoch in which reads are
re-typed as SCANs decides, grants, reads and writes exactly as before: the
formulas of tests/adversarial.py and tests/adversarial_calvin.py hold for it
unchanged, and they are the reference here.

`scan_substitute` re-types reads by POSITION only -- it looks at the epoch's
types and at nothing the case expects.  `reference` gives, from the family's
formula and the table's F0 column before the epoch, everything an epoch
computes: commit bytes, CALVIN's grant groups, the read digest, the write count
and F0 after it.  Neither the oracle nor the engine enters it.

The read digest (include/dvcc.h, dv_stats.read_digest) is the sum over the
committed RD and SCAN accesses of mix64(v ^ mix64(txn << 32 ^ key)), v the
value read.  Under NO_WAIT, WAIT_DIE and OCC a committed txn reads what the
row held before the epoch: an earlier committed write of the row would have
aborted it (a shared lock behind an exclusive one; a validation against the
writer's write set), an aborted txn's write is undone or never installed, and
its own earlier write of the row meets itself (H9) under locking, while OCC
reads the copy taken before any write.  A committed write stores 0.  Under
CALVIN adversarial_calvin's serial model gives the values.
"""
import copy
import dataclasses
import functools
from collections import namedtuple

import numpy as np

import adversarial as A
import adversarial_calvin as AC
import loop_cases as LC
from adversarial import RD, WR
from dvcc import Epoch
from index_cases import read_digest

SCAN = 3
PATTERNS = ("all", "mod3", "edge")
DECIDING = ("NO_WAIT", "WAIT_DIE", "OCC")
K = A.structural_constants()

Ref = namedtuple("Ref", "commit grant digest writes f0")


def _gather(tb, ids):
    """the access indices of txns `ids`, in that order"""
    tb = tb.astype(np.int64)
    ids = np.asarray(ids, np.int64)
    lens = tb[ids + 1] - tb[ids]
    start = np.r_[0, np.cumsum(lens)]
    return np.repeat(tb[ids] - start[:-1], lens) + np.arange(int(start[-1]), dtype=np.int64)


def scan_positions(types, pattern):
    """which accesses `pattern` re-types: reads only, picked by access index"""
    types = np.asarray(types, np.uint8)
    n = len(types)
    a = np.arange(n)
    if pattern == "all":
        pick = np.ones(n, bool)
    elif pattern == "mod3":
        pick = a % 3 == 0
    else:
        assert pattern == "edge" and n % 4, "the edge pattern wants an access count that is no multiple of 4"
        pick = a >= n - n % 4
    return pick & (types == RD)


def scan_substitute(case, pattern):
    """A copy of `case` (adversarial.Case or adversarial_calvin.CalvinCase) in
    which the reads `pattern` picks carry type DV_SCAN (3):
      all   every read
      mod3  the reads at access indices a with a % 3 == 0 (a 4-byte word of
            type bytes then mixes 0, 1 and 3)
      edge  the reads among the last n_acc % 4 accesses of the epoch (the
            accesses past the last whole 4-byte word of type bytes)
    Everything the case expects -- expected, grant, sees0, extra -- is the
    same object as before and is never looked at: a SCAN takes LOCK_SH as a
    RD does (row.cpp:191, :228) and reads the row as a RD does (row.cpp:257,
    ycsb_txn.cpp:228), so no expectation moves.  A carried epoch
    (case.carried, the aborted txns extra["carried_from"] in order) takes the
    bytes its accesses have in the substituted epoch."""
    e = case.epoch
    types = e.types.copy()
    types[scan_positions(types, pattern)] = SCAN
    out = dataclasses.replace(case, epoch=Epoch(e.keys, types, e.txn_begin, e.tables))
    carried = getattr(case, "carried", None)
    if carried is not None:
        idx = _gather(e.txn_begin, case.extra["carried_from"])
        assert np.array_equal(e.keys[idx], carried.keys)
        out.carried = Epoch(carried.keys, types[idx], carried.txn_begin)
    return out


def n_scans(case):
    return int((case.epoch.types == SCAN).sum())


def pad_reads(case, rem):
    """`case` with single-read txns appended, each of a row of its own past
    case.rows, until n_acc % 4 == rem: they conflict with nothing, so they
    commit under every algorithm, share no queue (grant 0) and see what their
    row held.  (For the edge pattern: the epoch's last rem accesses are then
    reads.)"""
    e = case.epoch
    n = (rem - e.n_acc) % 4
    n += 4 if n < rem else 0  # (at least rem of them: the whole edge is reads)
    keys = np.r_[e.keys, case.rows + np.arange(n, dtype=np.uint64)].astype(np.uint64)
    types = np.r_[e.types, np.zeros(n, np.uint8)]
    tb = np.r_[e.txn_begin, e.txn_begin[-1] + 1 + np.arange(n, dtype=np.uint32)].astype(np.uint32)
    new = dict(epoch=Epoch(keys, types, tb), rows=case.rows + n)
    if case.grant is not None:
        new["grant"] = np.r_[case.grant, np.zeros(n, np.uint32)]
    if isinstance(case, AC.CalvinCase):
        new["sees0"] = np.r_[case.sees0, np.zeros(n, bool)]
    else:
        new["expected"] = {cc: np.r_[c, np.ones(n, np.uint8)] for cc, c in case.expected.items()}
    out = dataclasses.replace(case, **new)
    assert out.epoch.n_acc % 4 == rem
    return out


# ---------------------------------------------------------------- the reference
def reference(case, cc, f0_before):
    """Ref(commit, grant, digest, writes, f0) of the case's epoch under `cc` on
    a table (row == key) whose rows hold f0_before, by the formulas alone;
    grant is None where the family states none"""
    e = case.epoch
    f0_before = np.asarray(f0_before, np.uint64)
    if isinstance(case, AC.CalvinCase):
        assert cc == "CALVIN"
        digest, writes, f0 = AC.outcome(case, f0_before)
        return Ref(np.ones(e.n_txn, np.uint8), case.grant, digest, writes, f0)
    commit = case.expected_commit(cc)
    if cc == "CALVIN":
        assert commit.all()
        grant, digest, writes, f0 = AC.serial_model(e, f0_before, np.arange(len(f0_before), dtype=np.uint64))
        if case.grant is not None:
            assert np.array_equal(grant, case.grant), "the serial model off the family's grant formula"
        return Ref(commit, case.grant, digest, writes, f0)
    txn = e.acc_txn()
    live = commit.astype(bool)[txn]
    wr = (e.types == WR) & live
    rd = (e.types != WR) & live  # RD and SCAN
    rows = e.keys.astype(np.int64)
    f0 = f0_before.copy()
    f0[rows[wr]] = 0
    return Ref(commit, None, read_digest(f0_before[rows[rd]], txn[rd], e.keys[rd]), int(wr.sum()), f0)


def held(ref, c, g, st, table, what):
    """one epoch's outcome against the formulas: commit bytes, grants where
    stated, the counts, the read digest and the F0 column"""
    bad = np.flatnonzero(np.asarray(c) != ref.commit)
    assert len(c) == len(ref.commit) and bad.size == 0, f"{what}: {bad.size} txns off the formula, first {bad[:8]}"
    if g is not None and ref.grant is not None:
        bad = np.flatnonzero(np.asarray(g) != ref.grant)
        assert bad.size == 0, f"{what}: {bad.size} grants off the formula, first at accesses {bad[:8]}"
    n = int(ref.commit.sum())
    assert (st.committed, st.aborted) == (n, len(ref.commit) - n), what
    assert st.write_cnt == ref.writes, f"{what}: write count {st.write_cnt}, formula {ref.writes}"
    assert st.read_digest == ref.digest, f"{what}: read digest {st.read_digest:#x}, closed form {ref.digest:#x}"
    if table is not None:
        bad = np.flatnonzero(np.asarray(table) != ref.f0)
        assert bad.size == 0, f"{what}: {bad.size} rows off the formula, first {bad[:8]}"


# ---------------------------------------------------------------- the families
def _sweep_rows():
    return 2 * K["kHotRows"] + 37


# name -> (builder, the algorithms its formulas cover): the small forms of the
# families in which a read decides something
FAMILIES = {
    # family 3: runs of m readers on one row at a wave's and a workgroup's edge
    "runs_63": (lambda: A.read_runs(63, 5), A.CCS),
    "runs_64": (lambda: A.read_runs(64, 5), A.CCS),
    "runs_65": (lambda: A.read_runs(65, 5), A.CCS),
    "runs_kBlock+1": (lambda: A.read_runs(K["kBlock"] + 1, 5), A.CCS),
    # family 2b: the readers wait behind the gate's write; both outcomes
    "gate_odd": (lambda: A.ladder_gate(301, 1204), A.CCS),
    "gate_even": (lambda: A.ladder_gate(300, 1200), A.CCS),
    # family 2: the even ladder txns read the hot row the odd ones write
    "ladder_hot": (lambda: A.ladder_hot(301, 5), A.CCS),
    # family 4: every txn writes row 0 and reads a private row
    "storm": (lambda: A.writer_storm(K["kBlock"] + 1), A.CCS),
    # family 5: 127 reads of one row, then a read / a write of it (H9), then a reader
    "self_R": (lambda: A.self_conflict(RD), A.CCS),
    "self_W": (lambda: A.self_conflict(WR), A.CCS),
    # family 6: the sweep reads every row, the prefix reads and writes some
    "sweep_1": (lambda: A.row_sweep(_sweep_rows(), 512, 0, 1), DECIDING),
    "sweep_63": (lambda: A.row_sweep(_sweep_rows(), 512, 0, 63), DECIDING),
    # family 8 with private reads: the aborted txns' reads are carried
    "carry_ladder": (lambda: A.ladder(301, empties=True, reads=True), A.CCS),
    "carry_blocks": (lambda: A.carry_blocks(K["kBlock"], reads=True), DECIDING),
}
CARRIED = ("carry_ladder", "carry_blocks")
SWEEP_PREFIX = 512


@functools.lru_cache(maxsize=None)
def family(name):
    return FAMILIES[name][0]()


@functools.lru_cache(maxsize=None)
def substituted(name, pattern):
    """family `name` under `pattern`, padded for the edge pattern so that its
    last 1, 2 or 3 accesses (in turn over the families) are reads; it holds
    at least one SCAN"""
    case = family(name)
    if pattern == "edge":
        case = pad_reads(case, 1 + list(FAMILIES).index(name) % 3)
    out = scan_substitute(case, pattern)
    assert n_scans(out) > 0, (name, pattern)
    if pattern == "edge":
        assert n_scans(out) == out.epoch.n_acc % 4 and (out.epoch.types[-n_scans(out):] == SCAN).all()
    return out


def _hidden(x0=1):
    return [AC.hidden_write(m, x0 + i) for i, m in enumerate(AC.hidden_write_sizes())]


# CALVIN's own families, in batches that run one after the other on one table
# (every case on hot rows of its own, the F0 column carried by the formula)
CALVIN_BATCHES = {
    "repeat_kPV": lambda: AC.repeat_blocks(AC.REPEAT_B["kPV"]),
    "repeat_kRTile": lambda: AC.repeat_blocks(AC.REPEAT_B["kRTile"]),
    "hidden": _hidden,
    "comb": AC.comb_epochs,
    "runs_storm": lambda: [AC.read_runs(K["kRTile"] + 1, 3), AC.writer_storm(K["kRTile"] + 1)],
}


@functools.lru_cache(maxsize=None)
def calvin_batch(name, pattern):
    """(cases, rows): the batch under `pattern`.  The edge pattern's padding
    reads rows past every case's own (rows the batch never writes)."""
    cases = CALVIN_BATCHES[name]()
    rows = max(c.rows for c in cases)
    out = []
    for i, case in enumerate(cases):
        if pattern == "edge":
            case = pad_reads(dataclasses.replace(case, rows=rows), 1 + i % 3)
        out.append(scan_substitute(case, pattern))
    assert all(n_scans(c) > 0 for c in out), (name, pattern)
    return out, max(c.rows for c in out)


def batch_references(cases, rows, calls=1):
    """the batch's epochs in sequence, `calls` times over, on one fresh table:
    a Ref per epoch"""
    f0 = AC.initial_f0(rows)
    out = []
    for _ in range(calls):
        for case in cases:
            out.append(reference(case, "CALVIN", f0))
            f0 = out[-1].f0
    return out


# ---------------------------------------------------------------- the partitioned shape
def part_ladder(world=2):
    """test_partitioned_ladder's shape with reads in it: 301 ladder txns [W k,
    W k+1] with two private accesses each (a write, then reads, in turn: family
    9), padded with empty txns to a multiple of `world` txns.  Key k lives on
    partition k % world, so every ladder txn spans two partitions."""
    case = A.ragged_ladder([2] * 301 + [A.EMPTY] * (-301 % world), 1, lambda k: k)
    assert case.epoch.n_txn % world == 0 and (case.epoch.types == RD).sum() > 300
    return case


# ---------------------------------------------------------------- the closed loop's pool
LOOP_N = 9 * K["kBlock"]  # the smallest epoch loop_cases' hot-row pool takes: nine carry blocks
LOOP_EPOCHS = 4


@functools.lru_cache(maxsize=None)
def loop_pool(pattern):
    """loop_cases' hot-row pool (txns of 0 .. 3 accesses: write, read, write)
    for epochs of LOOP_N txns, its reads re-typed; the commit formula
    (loop_cases.formula) never looks at a type byte of a read"""
    p = copy.copy(LC.HotPool((LOOP_EPOCHS + 1) * LOOP_N, LOOP_N, "mod4"))
    e = p.epoch
    types = e.types.copy()
    types[scan_positions(types, pattern)] = SCAN
    p.epoch = Epoch(e.keys, types, e.txn_begin)
    assert (types == SCAN).any()
    return p


def loop_epoch_reference(p, cc, src, f0_before):
    """the Ref of the epoch of pool txns `src`: loop_cases' commit formula, then
    `reference`"""
    host = LC.epoch_of(p, src)
    return reference(A.Case(host, p.rows, {cc: LC.formula(p.hw[src])}), cc, f0_before), host
