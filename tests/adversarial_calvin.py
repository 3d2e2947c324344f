"""Closed-form CALVIN epochs (a plain module, shared by
test_adversarial_calvin_cpu.py and test_adversarial_calvin_gpu.py).

Every CALVIN txn commits, so what an epoch computes is the grant group of each
access, the value each read sees, the write count and the F0 column after it.
The rule (the lock thread queues the whole epoch in sequence order, the workers
always run the lowest-sequence ready txn, which is always ready: execution is
serial in sequence order, a txn's reads before its own writes):

  grants  per row, one queue entry per txn in sequence order, typed by the
          txn's FIRST access to the row (TxnManager::get_lock, txn.cpp:778-788);
          a new group starts when the entry or the one before it is EX; a repeat
          access takes the grant of its txn's first access to the row
  values  a read sees 0 iff an earlier txn of this epoch wrote the row or the
          row already held 0, else the row's value before the epoch; a txn
          never sees its own writes
  writes  every write access counts; a written row holds 0 afterwards

`serial_model` is that rule in plain Python.  Every family below states its
grants and the set of reads that see 0 by a formula of its own, written
directly; `outcome` turns a formula into digest, write count and F0.  Nothing
here is taken from the oracle or the engine: both are held to it.

The families are sized by the row-queue kernels' geometry (structural_constants:
kPV, kRIPT, kRTile, kBlock, kMaxPos).  Row 0 only ever takes filler reads, so
it sorts first and `shift` fillers put the next row's queue at sorted position
`shift`.  Every case has hot rows of its own, so an earlier epoch on the same
table leaves their initial values alone.
"""
from dataclasses import dataclass, field

import numpy as np

import adversarial as A
from adversarial import RD, WR, _mk
from index_cases import read_digest, ycsb_f0

K = A.structural_constants()


@dataclass
class CalvinCase:
    name: str
    epoch: object                # dvcc.Epoch
    rows: int                    # the table has to hold rows [0, rows)
    grant: np.ndarray            # uint32 [n_acc], the formula's grant groups
    sees0: np.ndarray            # bool [n_acc]: the reads that see 0 whatever the row held (False at a write)
    extra: dict = field(default_factory=dict)


def initial_f0(rows):
    """the F0 column a fresh YCSB table of `rows` rows holds (row == key)"""
    return np.array([ycsb_f0(k) for k in range(rows)], np.uint64)


def rows_of(keys, pkey):
    """the row of every key under `pkey` (pkey[row] = the row's key)"""
    pkey = np.asarray(pkey, np.uint64)
    order = np.argsort(pkey, kind="stable")
    at = np.searchsorted(pkey[order], keys)
    rows = order[np.minimum(at, len(pkey) - 1)]
    assert np.array_equal(pkey[rows], keys), "a key without a row"
    return rows.astype(np.int64)


def sorted_order(e, pkey=None):
    """the accesses' order in the row queues: by row, then sequence (txn, then
    position in the txn)"""
    rows = rows_of(e.keys, pkey) if pkey is not None else e.keys.astype(np.int64)
    return np.lexsort((np.arange(e.n_acc), e.acc_txn().astype(np.int64), rows))


# ---------------------------------------------------------------- the model
def serial_model(epoch, f0_before, pkey):
    """(grant [n_acc], read digest, write count, F0 after) of `epoch` on a table
    whose rows hold f0_before and have the keys pkey -- the rule of the module's
    docstring, txn by txn"""
    e = epoch
    rows = rows_of(e.keys, pkey)
    tb = e.txn_begin.astype(np.int64)
    types = e.types
    grant = np.zeros(e.n_acc, np.uint32)
    last = {}           # row -> (group, EX) of its queue's last entry
    written = set()     # rows an earlier txn wrote
    values = np.zeros(e.n_acc, np.uint64)
    writes = 0
    for t in range(e.n_txn):
        mine = {}       # row -> this txn's grant on it
        for a in range(tb[t], tb[t + 1]):
            r = int(rows[a])
            if r not in mine:
                ex = types[a] == WR
                if r in last:
                    g, prev_ex = last[r]
                    g += 1 if (ex or prev_ex) else 0
                else:
                    g = 0
                last[r] = (g, ex)
                mine[r] = g
            grant[a] = mine[r]
        for a in range(tb[t], tb[t + 1]):
            r = int(rows[a])
            if types[a] != WR:  # RD, SCAN
                values[a] = 0 if (r in written or f0_before[r] == 0) else f0_before[r]
        for a in range(tb[t], tb[t + 1]):
            if types[a] == WR:
                writes += 1
                written.add(int(rows[a]))
    rd = types != WR
    digest = read_digest(values[rd], e.acc_txn()[rd], e.keys[rd])
    f0 = np.array(f0_before, np.uint64, copy=True)
    f0[sorted(written)] = 0
    return grant, digest, writes, f0


def outcome(case, f0_before, pkey=None):
    """(read digest, write count, F0 after) a case's formula gives on a table
    that holds f0_before: a read the formula marks sees 0, every other read
    what its row held"""
    e = case.epoch
    rows = rows_of(e.keys, pkey) if pkey is not None else e.keys.astype(np.int64)
    rd = e.types != WR  # RD and SCAN: both read the row (ycsb_txn.cpp:228)
    assert not case.sees0[~rd].any()
    values = np.where(case.sees0, np.uint64(0), np.asarray(f0_before, np.uint64)[rows])
    digest = read_digest(values[rd], e.acc_txn()[rd], e.keys[rd])
    f0 = np.array(f0_before, np.uint64, copy=True)
    f0[rows[~rd]] = 0
    return digest, int((~rd).sum()), f0


def padded(case, n_txn):
    """the case with empty txns appended up to n_txn txns (they commit and
    change nothing: grants and values stay)"""
    return CalvinCase(case.name, A.pad_tail(case.epoch, n_txn), case.rows, case.grant, case.sees0, case.extra)


# ---------------------------------------------------------------- repeat block
# (B, reps, first, where).  `shift` txns [R 0], then P = [R x], then A, then
# Q = [R x], Z = [W x], Q2 = [R x].  A touches x `reps` times: its first access
# is of type `first`, its last a W, the others R.
#   grants  P 0.  first = R: A's entry is SH, it shares P's group 0 and Q shares
#           it too (A's later W does not retype the entry).  first = W: A 1,
#           Q 2.  Z and Q2 each open a new group.  Fillers 0.
#   values  P and A's reads see the initial value (A's own writes are not
#           seen); Q and Q2 see 0.
# In the row queues x's queue starts at sorted position `shift` (P) and A's run
# is [shift + 1, shift + reps].  E is the first multiple of B that leaves room
# for the run and P in front of it; `where` puts the run
#   start         first access at E               (the run opens a chunk)
#   end           last access at E - 1            (the run closes a chunk)
#   first_before  first access at E - 1, the rest from E on
#   last_after    last access at E, the rest before it
REPEAT_B = {"kPV": K["kPV"],                       # a thread of k_seg_prepare / k_exec
            "wave": 64 * K["kPV"],                 # a wave of k_seg_prepare (lane 0 reads its predecessor from memory)
            "block": K["kBlock"] * K["kPV"],       # a workgroup's chunk of k_seg_prepare / k_exec
            "kRIPT": K["kRIPT"],                   # a thread of k_calvin_pass
            "kRTile": K["kRTile"]}                 # a tile of k_calvin_pass (the look-back)
REPEAT_REPS = (2, 3, K["kMaxPos"] - 4)
REPEAT_WHERE = ("start", "end", "first_before", "last_after")


def repeat_block(B, reps, first, where, x):
    assert reps >= 2 and reps + 4 <= K["kMaxPos"] and x >= 1
    E = -(-(reps + 1) // B) * B
    a0 = {"start": E, "end": E - reps, "first_before": E - 1, "last_after": E - reps + 1}[where]
    shift = a0 - 1
    assert shift >= 0
    a_types = [first] + [RD] * (reps - 2) + [WR]
    lens = np.r_[np.ones(shift + 1, np.int64), reps, 1, 1, 1]
    keys = np.r_[np.zeros(shift, np.int64), np.full(reps + 4, x, np.int64)]
    types = np.r_[np.zeros(shift + 1, np.uint8), np.uint8(a_types), np.uint8([RD, WR, RD])]
    e = _mk(lens, keys, types)
    gA = 1 if first == WR else 0
    gQ = 2 if first == WR else 0
    grant = np.r_[np.zeros(shift + 1, np.int64), np.full(reps, gA), gQ, gQ + 1, gQ + 2].astype(np.uint32)
    sees0 = np.zeros(e.n_acc, bool)
    sees0[shift + 1 + reps] = sees0[shift + 1 + reps + 2] = True  # Q, Q2
    # the run lies where intended, from the epoch alone
    pos = np.empty(e.n_acc, np.int64)
    pos[sorted_order(e)] = np.arange(e.n_acc)
    run = pos[shift + 1:shift + 1 + reps]
    assert np.array_equal(run, np.arange(a0, a0 + reps)) and pos[shift] == a0 - 1 and E % B == 0
    assert {"start": run[0] == E, "end": run[-1] == E - 1, "first_before": run[0] == E - 1 and run[1] == E,
            "last_after": run[-1] == E and run[-2] == E - 1}[where]
    return CalvinCase(f"repeat_B{B}_reps{reps}_{'RW'[first]}_{where}", e, x + 1, grant, sees0,
                      extra=dict(B=B, edge=E, run=(int(run[0]), int(run[-1])), hot=x))


def repeat_blocks(B, x0=1):
    """every (reps, first, where) of one B, hot rows x0, x0 + 1, ...
    (`last_after` is `first_before` again at reps = 2 and left out there)"""
    out = []
    for reps in REPEAT_REPS:
        for first in (RD, WR):
            for where in REPEAT_WHERE:
                if reps == 2 and where == "last_after":
                    continue
                out.append(repeat_block(B, reps, first, where, x0 + len(out)))
    return out


# ---------------------------------------------------------------- hidden write
# (m).  m txns [R x], then one txn [R x, W x], then m txns [R x].  The middle
# txn's entry is typed by its first access, a read: all 2m + 1 entries share
# group 0 (and the W, a repeat, takes that grant).  The first m readers and
# the middle txn's own read see the initial value, the last m readers see 0.
# No boundary follows the queue's head, so the boundary count a tile of
# k_calvin_pass hands on through the look-back stays 0 while its seen-a-write
# bit has to travel.
def hidden_write_sizes():
    T = K["kRTile"]
    return [T - 1, T, T + 1, 3 * T + 5]


def hidden_write(m, x, shift=0):
    lens = np.r_[np.ones(shift + m, np.int64), 2, np.ones(m, np.int64)]
    keys = np.r_[np.zeros(shift, np.int64), np.full(2 * m + 2, x, np.int64)]
    types = np.zeros(shift + 2 * m + 2, np.uint8)
    types[shift + m + 1] = WR
    e = _mk(lens, keys, types)
    sees0 = np.zeros(e.n_acc, bool)
    sees0[shift + m + 2:] = True
    return CalvinCase(f"hidden_write_{m}", e, x + 1, np.zeros(e.n_acc, np.uint32), sees0,
                      extra=dict(write_at=shift + m + 1, hot=x))


# ---------------------------------------------------------------- queue comb
# Eight short queues, written by hand: the queue's txns in sequence order (each
# a list of access types), the grant of every access and whether it sees 0
# (None at a write).
_R, _W, _N = RD, WR, None
COMB = (
    ([[_R]],             [0],        [False]),
    ([[_W]],             [0],        [_N]),
    ([[_R], [_R]],       [0, 0],     [False, False]),
    ([[_R], [_W]],       [0, 1],     [False, _N]),
    ([[_W], [_R]],       [0, 1],     [_N, True]),
    ([[_W], [_W]],       [0, 1],     [_N, _N]),
    ([[_R, _W], [_R]],   [0, 0, 0],  [False, _N, True]),   # the entry stays SH; the W is hidden in group 0
    ([[_W, _R], [_R]],   [0, 0, 1],  [_N, False, True]),   # the txn's read does not see its own write
)


def comb(R, row0, shift=0, reverse=False):
    """Rows row0 + 1 .. row0 + R; row row0 + r takes COMB[r % 8].  `shift`
    txns [R 0] first, then every queue's first txn, row by row, then every
    queue's second txn, row by row -- in rising row order, or (reverse) in
    falling row order, so that sequence order and row order differ."""
    rs = list(range(1, R + 1))
    if reverse:
        rs.reverse()
    lens, keys, types, grant, sees0 = [1] * shift, [0] * shift, [RD] * shift, [0] * shift, [False] * shift
    for slot in (0, 1):
        for r in rs:
            txns, g, s = COMB[r % 8]
            if slot >= len(txns):
                continue
            a = sum(len(t) for t in txns[:slot])
            n = len(txns[slot])
            lens.append(n)
            keys += [row0 + r] * n
            types += txns[slot]
            grant += g[a:a + n]
            sees0 += [bool(v) for v in s[a:a + n]]
    e = _mk(np.array(lens, np.int64), np.array(keys, np.int64), np.array(types, np.uint8))
    return CalvinCase(f"comb_{R}_s{shift}{'_rev' if reverse else ''}", e, row0 + R + 1,
                      np.array(grant, np.uint32), np.array(sees0, bool), extra=dict(R=R, row0=row0, shift=shift))


def _comb_acc(R):
    return sum(sum(len(t) for t in COMB[r % 8][0]) for r in range(1, R + 1))


def comb_epochs(row0=0):
    """the comb's epochs on disjoint row ranges: R = 2 kRTile + d, d = 0 .. 3,
    with fillers so that the access count is d mod kPV (k_exec's scalar tail
    and its full vectors); R = 2 kRTile + 37 in rising and in falling row
    order, shifted so that over the epochs the queue heads fall on every
    position of a thread's kRIPT entries and of its kPV accesses"""
    T, pv = K["kRTile"], K["kPV"]
    out = []
    for d in range(4):
        R = 2 * T + d
        c = comb(R, row0, shift=(d - _comb_acc(R)) % pv)
        assert c.epoch.n_acc % pv == d % pv
        out.append(c)
        row0 += R + 1
    for shift, rev in ((5, False), (6, True)):
        out.append(comb(2 * T + 37, row0, shift=shift, reverse=rev))
        row0 += 2 * T + 37 + 1
    return out


def head_positions(case):
    """the sorted positions of the queue heads of a case's epoch"""
    e = case.epoch
    order = sorted_order(e)
    rows = e.keys[order]
    return np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])


# ---------------------------------------------------------------- families 3 and 4
def read_runs(m, r):
    """adversarial.read_runs with its values: run 0's readers see the initial
    value, every later reader sees 0"""
    c = A.read_runs(m, r)
    run = np.arange(c.epoch.n_acc) // (m + 1)
    return CalvinCase(f"read_runs_{m}x{r}", c.epoch, c.rows, c.grant, (c.epoch.types == RD) & (run > 0))


def writer_storm(n):
    """adversarial.writer_storm with its values: the private reads see the
    initial value"""
    c = A.writer_storm(n)
    return CalvinCase(f"writer_storm_{n}", c.epoch, c.rows, c.grant, np.zeros(c.epoch.n_acc, bool))
