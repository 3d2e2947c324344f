"""Closed-form adversarial epochs (a plain module, shared by
test_adversarial_cpu.py and test_adversarial_gpu.py).

Every generator builds an epoch whose commit set follows from the reference's
rules by a formula one can check by hand, and returns a `Case`: the epoch, the
rows its table needs and, per CC algorithm, `expected_commit` -- a uint8 array
computed here in numpy, never taken from the oracle or the engine.  Both are
then held to it.

The rules used (E-schedule, SURVEY.md 8.0: txns decide in sequence order, a
committed txn holds its locks / stays in the validation history to the end of
the epoch, an aborted one leaves nothing behind):
  NO_WAIT / WAIT_DIE  an access aborts its txn when an earlier committed txn
                      holds a conflicting lock on the row (row_lock.cpp:52-217;
                      timestamps rise with sequence order, so WAIT_DIE's
                      younger requester dies where NO_WAIT's aborts), and when
                      the txn's own earlier access does (hazard H9)
  OCC                 a txn aborts when an earlier committed txn wrote a row
                      it accesses (occ.cpp:116-239; writes are read-modify-
                      write, so they are validated like reads)
  CALVIN              every txn commits; a row's accesses are granted in
                      sequence order in groups, a run of reads sharing one
                      group (txn.cpp:778-788)
W = write, R = read below; each k names a distinct row unless stated.
"""
import os
import re
from dataclasses import dataclass, field

import numpy as np

from dvcc import Epoch

CCS = ("NO_WAIT", "WAIT_DIE", "OCC", "CALVIN")
LOCKING = ("NO_WAIT", "WAIT_DIE")
RD, WR = 0, 1


@dataclass
class Case:
    epoch: Epoch
    rows: int
    expected: dict                              # cc name -> uint8 [n_txn]
    grant: np.ndarray = None                    # CALVIN grant groups [n_acc] where a formula is given
    carried: Epoch = None                       # family 8: the epoch the aborted txns form (locking + OCC)
    extra: dict = field(default_factory=dict)

    def expected_commit(self, cc):
        return self.expected[cc]


def _mk(lens, keys, types):
    tb = np.zeros(len(lens) + 1, np.uint32)
    tb[1:] = np.cumsum(lens)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    types = np.ascontiguousarray(types, dtype=np.uint8)
    assert int(tb[-1]) == len(keys) == len(types)
    return Epoch(keys, types, tb)


def _ones(n):
    return np.ones(n, np.uint8)


# ---- the structural constants the cases are sized by, read from the source
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva-plus_amd", "csrc")


def _src(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _define(text, name):
    """a `#define NAME value` default, or its -DNAME=value override of the
    build (DVCC_DEFINES, deneva-plus_amd/build.py)"""
    for d in os.environ.get("DVCC_DEFINES", "").split():
        m = re.fullmatch(r"-D%s=(\d+)" % name, d)
        if m:
            return int(m.group(1))
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def _const(text, name):
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)" % name, text).group(1))


def structural_constants():
    """kTile (the synchronous pass's tile of 32-bit elements and of 64-bit
    ones), kAsyncCap, the tail capacities, kBlock / kCarryTpb, kHotRows and
    the Bloom filter's bits, and the partitioned path's kXTile (a tile of
    landed accesses), kOwnerTile (the owner split's tile of home accesses:
    dvcc_internal.h's kTile, the radix kernels'), kIlTxns / kIlOwn
    (k_il_move_tb's tile of txns and its LDS index), kMaxPos (the longest txn)
    and kRouteBlocks, and the row-queue kernels' kPV (consecutive accesses of
    a thread of k_seg_prepare / k_exec), kRIPT and kRTile (a thread's entries
    and a workgroup's tile of k_calvin_pass), from csrc/."""
    rounds, internal, prefix = _src("dvcc_rounds.hip"), _src("dvcc_internal.h"), _src("dvcc_prefix.hip")
    comm, kernels, common = _src("dvcc_comm.hip"), _src("dvcc_kernels.hip"), _src("dvcc_common.h")
    assert re.search(r"constexpr\s+uint32_t\s+kXTile\s*=\s*kBlock\s*\*\s*kXIPT\s*;", comm)
    assert re.search(r"constexpr\s+int\s+kRTile\s*=\s*kBlock\s*\*\s*kRIPT\s*;", common)
    assert re.search(r"constexpr\s+int\s+kTile\s*=\s*kBlock\s*\*\s*kIPT\s*;", internal)
    il = re.search(r"constexpr\s+uint32_t\s+kIlTxns\s*=\s*(\d+)\s*,\s*kIlOwn\s*=\s*(\d+)\s*;", comm)
    max_pos = re.search(r"constexpr\s+uint32_t\s+kMaxPos\s*=\s*1u\s*<<\s*(\d+)\s*;", internal)
    t32 = int(re.search(r"kThreads\s*=\s*sizeof\(EIn\)\s*==\s*4\s*\?\s*(\d+)", rounds).group(1))
    tail = re.search(r"struct TailGeo\s*\{\s*static constexpr int kIPT = sizeof\(E\) == 4 \? (\d+) : (\d+);", rounds)
    tail_threads = _const(internal, "kTailThreads")
    async_threads = _const(rounds, "kAsyncThreads")
    return dict(
        kBlock=_const(internal, "kBlock"),
        kAsyncThreads=async_threads,
        kTile=t32 * _define(rounds, "DVCC_ROUND_IPT"),
        kTile64=_define(rounds, "DVCC_ROUND_T64") * _define(rounds, "DVCC_ROUND_IPT64"),
        kAsyncCap=async_threads * _define(rounds, "DVCC_ASYNC_IPT"),
        kTailCap32=tail_threads * int(tail.group(1)),
        kTailCap64=tail_threads * int(tail.group(2)),
        kHotRows=1 << _define(prefix, "DVCC_HOT_LOG"),
        kBloomBits=1 << _define(prefix, "DVCC_BLOOM_LOG"),
        kRoundLog=_const(internal, "kRoundLog"),
        kXTile=_const(internal, "kBlock") * _const(comm, "kXIPT"),
        kOwnerTile=_const(internal, "kBlock") * _const(internal, "kIPT"),
        kIlTxns=int(il.group(1)),
        kIlOwn=int(il.group(2)),
        kMaxPos=1 << int(max_pos.group(1)),
        kRouteBlocks=_const(internal, "kRouteBlocks"),
        kPV=_const(kernels, "kPV"),
        kRIPT=_const(common, "kRIPT"),
        kRTile=_const(internal, "kBlock") * _const(common, "kRIPT"),
    )


# ---- family 1: Ladder(L).  T_k = [W k, W k+1], k < L.
# NO_WAIT / WAIT_DIE / OCC: T_0 commits, T_1 meets T_0's lock (write) on row 1
# and aborts, T_2 then finds row 2 free ... T_k commits iff k is even.
# CALVIN: all commit.  A dependency chain L deep: T_k's verdict needs T_{k-1}'s.
# reads=True: T_k = [W k, W k+1] + 1 + k % 2 reads of private rows (L + 1 on,
# each read once in the whole epoch).  A private read conflicts with nothing,
# so every formula stays; the carried txns carry their reads along.
def _ladder_arrays(k, L, reads):
    """(lens, keys, types) of ladder txns k, private rows as in the whole ladder"""
    nr = (1 + k % 2) if reads else np.zeros(len(k), np.int64)
    priv0 = L + 1 + k + k // 2  # (1 + j % 2 summed over j < k)
    lens = 2 + nr
    tb = np.r_[0, np.cumsum(lens)]
    txn = np.repeat(np.arange(len(k)), lens)
    j = np.arange(int(tb[-1])) - tb[txn]
    keys = np.where(j < 2, k[txn] + j, priv0[txn] + j - 2)
    return lens, keys, (j < 2).astype(np.uint8)


def ladder(L, empties=False, reads=False):
    k = np.arange(L, dtype=np.int64)
    lens, keys, types = _ladder_arrays(k, L, reads)
    even = (k % 2 == 0).astype(np.uint8)
    if empties:  # family 8: an empty txn after every ladder txn (empties commit)
        lens = np.stack([lens, np.zeros(L, np.int64)], 1).ravel()
        even = np.stack([even, _ones(L)], 1).ravel()
    e = _mk(lens, keys, types)
    exp = {cc: even.copy() for cc in LOCKING + ("OCC",)}
    exp["CALVIN"] = _ones(e.n_txn)
    # the aborted txns, in order and renumbered from 0: the odd ladder txns,
    # L // 2 of them with their accesses unchanged; they touch disjoint rows
    # (k, k+1 for odd k, and private ones), so run as the next epoch all of
    # them commit
    odd = k[1::2]
    carried = _mk(*_ladder_arrays(odd, L, reads))
    return Case(e, L + 1 + (int(lens.sum()) - 2 * L if reads else 0), exp, carried=carried,
                extra=dict(carried_from=odd * (2 if empties else 1)))


# ---- family 2: Ladder + hot row(L, f).  Ladder txn k = [X hot, W k, W k+1],
# X = R for even k and W for odd k, each followed by f txns [R hot].
# The ladder decides as in family 1 (the odd txns abort on row k, so their
# write of the hot row never holds): ladder txn k commits iff k is even, and
# no writer of the hot row commits, so every reader of it -- the even ladder
# txns and every pure reader -- commits.  Under OCC each hot read waits on the
# undecided writers before it, so the hot queue stays live for about L steps
# (NO_WAIT / WAIT_DIE: see family 2b).
def _ladder_hot_arrays(L, f, hot, row0):
    k = np.arange(L, dtype=np.int64)
    g = 3 + f  # accesses per group
    keys = np.full((L, g), hot, np.int64)
    keys[:, 1], keys[:, 2] = row0 + k, row0 + k + 1
    types = np.zeros((L, g), np.uint8)
    types[:, 0] = k % 2
    types[:, 1:3] = 1
    lens = np.ones((L, 1 + f), np.int64)
    lens[:, 0] = 3
    commit = np.ones((L, 1 + f), np.uint8)
    commit[:, 0] = k % 2 == 0
    return lens.ravel(), keys.ravel(), types.ravel(), commit.ravel()


def ladder_hot(L, f):
    lens, keys, types, commit = _ladder_hot_arrays(L, f, hot=0, row0=1)
    e = _mk(lens, keys, types)
    exp = {cc: commit.copy() for cc in LOCKING + ("OCC",)}
    exp["CALVIN"] = _ones(e.n_txn)
    return Case(e, L + 2, exp, extra=dict(hot_share=(L * (1 + f)) / e.n_acc))


# ---- family 2b: Ladder gate(L, n).  Under NO_WAIT / WAIT_DIE family 2's odd
# ladder txns die on T_0's committed read of the hot row within a few rounds
# (a write conflicts with ANY earlier committed access), so only OCC keeps its
# hot queue undecided for L steps.  This variant holds for every algorithm:
# family 1's ladder, whose LAST txn also writes the hot row, then n txns
# [R hot].  Nothing touches the hot row before that write, which stays
# undecided until the ladder reaches it (L - 1 steps), and all n reads wait
# behind it.  Ladder txn k commits iff k is even; the readers commit iff the
# gate txn L - 1 aborts, i.e. iff L is even.  CALVIN: all commit.
def ladder_gate(L, n):
    k = np.arange(L, dtype=np.int64)
    keys = np.r_[np.stack([1 + k, 2 + k], 1).ravel(), np.zeros(1 + n, np.int64)]
    types = np.r_[_ones(2 * L + 1), np.zeros(n, np.uint8)]
    lens = np.r_[np.full(L - 1, 2), 3, np.ones(n, np.int64)]
    e = _mk(lens, keys, types)
    c = np.r_[(k % 2 == 0).astype(np.uint8), np.full(n, L % 2 == 0, np.uint8)]
    exp = {cc: c.copy() for cc in LOCKING + ("OCC",)}
    exp["CALVIN"] = _ones(e.n_txn)
    return Case(e, L + 2, exp, extra=dict(hot_share=(1 + n) / e.n_acc))


# ---- family 3: Read runs(m, r).  One row; r times: m single-access readers,
# then one single-access writer.
# NO_WAIT / WAIT_DIE: the first run's readers commit and hold shared locks, so
# every writer aborts and every reader commits.
# OCC: the first run's readers commit, the first writer commits (earlier
# committed READS never invalidate), every later txn accesses a row a
# committed txn wrote: abort.
# CALVIN: all commit; grant group of run j's readers 2j, of its writer 2j + 1.
def read_runs(m, r):
    types = np.tile(np.r_[np.zeros(m, np.uint8), np.uint8(1)], r)
    n = len(types)
    e = _mk(np.ones(n, np.int64), np.zeros(n, np.int64), types)
    lock = (1 - types).astype(np.uint8)
    occ = np.zeros(n, np.uint8)
    occ[:m + 1] = 1
    run = np.arange(n) // (m + 1)
    return Case(e, 16, {"NO_WAIT": lock, "WAIT_DIE": lock.copy(), "OCC": occ, "CALVIN": _ones(n)},
                grant=(2 * run + types).astype(np.uint32))


# ---- family 4: Writer storm(n).  T_k = [W 0, R (10 + k)].
# NO_WAIT / WAIT_DIE / OCC: T_0 commits and every later txn writes the row it
# wrote: only T_0 commits.  CALVIN: all commit; row 0's grant groups are
# 0..n-1 (every writer its own group), the private reads get 0.
def writer_storm(n):
    k = np.arange(n, dtype=np.int64)
    e = _mk(np.full(n, 2), np.stack([np.zeros(n, np.int64), 10 + k], 1).ravel(), np.tile(np.uint8([1, 0]), n))
    one = np.zeros(n, np.uint8)
    one[0] = 1
    exp = {cc: one.copy() for cc in LOCKING + ("OCC",)}
    exp["CALVIN"] = _ones(n)
    return Case(e, 10 + n, exp, grant=np.stack([k, np.zeros(n, np.int64)], 1).ravel().astype(np.uint32))


# ---- family 5: self-conflict at the longest txn.  [R 3] x 127 + [X 3], then
# [R 3].
# X = R: nothing conflicts, both commit under every algorithm.
# X = W: NO_WAIT / WAIT_DIE: the first txn's write meets its own read locks
# (H9, row_lock.cpp:69, 86-90) and it aborts; the second then commits.
# OCC: a txn never conflicts with itself, the first commits having written row
# 3, the second reads it: abort.  CALVIN: both commit.
def self_conflict(x):
    types = np.zeros(129, np.uint8)
    types[127] = x
    e = _mk([128, 1], np.full(129, 3), types)
    both = _ones(2)
    if x == RD:
        exp = {cc: both.copy() for cc in CCS}
    else:
        exp = {"NO_WAIT": np.uint8([0, 1]), "WAIT_DIE": np.uint8([0, 1]), "OCC": np.uint8([1, 0]), "CALVIN": both}
    return Case(e, 8, exp)


# ---- family 6: Row sweep(rows, P, sweep_wr).  A prefix of P mutually
# disjoint txns (1..3 accesses each on distinct random rows, mixed types; rows
# kHotRows - 1, kHotRows, rows - 1 and rows - 38 forced in; the prefix's access
# count is `acc_mod` mod 64), then ceil(rows / 16) txns, txn j accessing rows
# 16j..16j+15, all reads (sweep_wr = 0) or all writes (1).
# The prefix txns touch disjoint rows: all commit.  The sweep txns are
# disjoint from one another too, so sweep txn j commits iff none of its rows
# is
#   written by the prefix             (NO_WAIT / WAIT_DIE read sweep; OCC both)
#   written or read by the prefix     (NO_WAIT / WAIT_DIE write sweep).
# The sweep touches every row once -- every row of every bitmap word, the
# partial last word, and every row that collides with a marked row in the
# Bloom filter.
def row_sweep(rows, P, sweep_wr, acc_mod, seed=6):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 4, size=P)
    short = np.flatnonzero(sizes < 3)[:(acc_mod - int(sizes.sum())) % 64]
    sizes[short] += 1
    n = int(sizes.sum())
    assert n % 64 == acc_mod
    hot = structural_constants()["kHotRows"]  # (the LDS copy holds rows [0, hot); the Bloom filter the rest)
    assert hot + 38 < rows, "the table has to reach past the hot rows"
    forced = np.array([hot - 1, hot, rows - 1, rows - 38], np.int64)
    pool = rng.permutation(rows)
    pool = pool[~np.isin(pool, forced)][:n]
    at = np.array([0, n // 3, n // 2, n - 1])
    pool[at] = forced
    ptypes = (rng.random(n) < 0.5).astype(np.uint8)
    ptypes[at] = [1, 1, 1, 0]
    nsweep = (rows + 15) // 16
    slens = np.full(nsweep, 16)
    slens[-1] = rows - 16 * (nsweep - 1)
    e = _mk(np.r_[sizes, slens], np.r_[pool, np.arange(rows, dtype=np.int64)],
            np.r_[ptypes, np.full(rows, sweep_wr, np.uint8)])
    wr = np.zeros(rows, bool)
    wr[pool[ptypes == 1]] = True
    any_acc = np.zeros(rows, bool)
    any_acc[pool] = True
    starts = np.arange(0, rows, 16)
    exp = {}
    for cc in LOCKING + ("OCC",):
        bad = any_acc if (sweep_wr and cc in LOCKING) else wr
        exp[cc] = np.r_[_ones(P), (np.add.reduceat(bad.astype(np.int64), starts) == 0).astype(np.uint8)]
    return Case(e, rows, exp, extra=dict(prefix_acc=n))


# ---- family 7: element-width boundary(n_txn).  n_txn - L - 1 filler txns
# each read one private row, one txn reads a single row 128 times (so slog = 7
# and a 32-bit element holds exactly 2^22 txns), then family 2 with f = 0 at
# the highest txn ids.  Fillers and the long txn conflict with nothing and
# commit; the ladder follows family 2's rule.
def width_boundary(n_txn, L=2001):
    F = n_txn - L - 1
    lens, keys, types, commit = _ladder_hot_arrays(L, 0, hot=F + 1, row0=F + 2)
    e = _mk(np.r_[np.ones(F, np.int64), 128, lens],
            np.r_[np.arange(F, dtype=np.int64), np.full(128, F), keys],
            np.r_[np.zeros(F + 128, np.uint8), types])
    assert e.n_txn == n_txn
    c = np.r_[_ones(F + 1), commit]
    return Case(e, F + 2 + L + 1, {cc: c.copy() for cc in ("NO_WAIT", "OCC")})


# ---- family 8: ladder with empties (ladder(L, empties=True)), and whole
# carry blocks of each kind.  carry_blocks(B): B txns per block --
#   block 0  B empty txns                              commit, nothing carried
#   block 1  [W k], k < B                              commit, nothing carried
#   block 2  [W k], k < B (block 1's rows again)       all abort, all carried
#   block 3  [W B + k], k < B                          commit, nothing carried
#   then 37 txns alternating [W B + i] (block 3's rows, abort) and empty.
# The carried epoch is block 2's txns then the 19 aborting ones of the last,
# partial block, in order, one write each on distinct rows: run as the next
# epoch they all commit.
# reads=True: every txn that is not empty reads a private row after its write
# (row 2 B + 8 + j for the j-th of them, read once in the whole epoch), which
# conflicts with nothing; the carried txns carry their reads along.
def carry_blocks(B, reads=False):
    k = np.arange(B, dtype=np.int64)
    tail_n = 37
    ti = np.arange((tail_n + 1) // 2, dtype=np.int64)
    tl = np.zeros(tail_n, np.int64)
    tl[0::2] = 1
    lens = np.r_[np.zeros(B, np.int64), np.ones(3 * B, np.int64), tl]
    keys = np.r_[k, k, B + k, B + ti]
    cj = np.r_[B + k, 3 * B + ti]  # the carried txns among the ones that are not empty
    ck = np.r_[k, B + ti]
    assert np.array_equal(keys[cj], ck)
    rows = 2 * B + 8
    types = _ones(len(keys))
    if reads:
        priv = rows + np.arange(len(keys), dtype=np.int64)
        ck = np.stack([ck, priv[cj]], 1).ravel()
        keys, types, lens = np.stack([keys, priv], 1).ravel(), np.tile(np.uint8([WR, RD]), len(keys)), 2 * lens
        rows += len(priv)
    e = _mk(lens, keys, types)
    c = np.r_[_ones(2 * B), np.zeros(B, np.uint8), _ones(B), (tl == 0).astype(np.uint8)]
    per = 2 if reads else 1
    carried = _mk(np.full(len(cj), per), ck, np.tile(types[:per], len(cj)))
    return Case(e, rows, {cc: c.copy() for cc in LOCKING + ("OCC",)}, carried=carried,
                extra=dict(carried_from=np.r_[2 * B + k, 4 * B + 2 * ti]))


def contiguous_chunks(e, world):
    """`e` cut into `world` contiguous chunks of ceil(n_txn / world) txns (the
    last one shorter), txn ids local to the chunk"""
    tpr = (e.n_txn + world - 1) // world
    tb = e.txn_begin.astype(np.int64)
    out = []
    for r in range(world):
        a, b = min(r * tpr, e.n_txn), min((r + 1) * tpr, e.n_txn)
        out.append(Epoch(e.keys[tb[a]:tb[b]].copy(), e.types[tb[a]:tb[b]].copy(),
                         (tb[a:b + 1] - tb[a]).astype(np.uint32)))
    return out, tpr


def strided_chunks(e, world):
    """`e` dealt out txn by txn: origin q gets sequence slots q, q + world,
    ... as its txns 0, 1, ... (ceil(n_txn / world) slots each, the last ones
    of the later origins missing when world does not divide n_txn), txn ids
    local to the chunk.  dvcc.sequence_position of the chunks is `e` again, as
    dvcc.sequence of contiguous_chunks (each padded to tpr txns) is."""
    tpr = (e.n_txn + world - 1) // world
    tb = e.txn_begin.astype(np.int64)
    lens = np.diff(tb)
    out = []
    for q in range(world):
        ids = np.arange(q, e.n_txn, world)
        ltb = np.zeros(len(ids) + 1, np.int64)
        ltb[1:] = np.cumsum(lens[ids])
        idx = np.repeat(tb[ids] - ltb[:-1], lens[ids]) + np.arange(int(ltb[-1]))
        out.append(Epoch(e.keys[idx].copy(), e.types[idx].copy(), ltb.astype(np.uint32)))
    return out, tpr


def trim_tail(b):
    """`b` without its trailing empty txns: the batch an origin hands over
    when its last sequence slots hold no txn (its real, smaller n_txn, down to
    0); the slots it leaves are empty txns of the epoch, which commit."""
    n = np.flatnonzero(np.diff(b.txn_begin.astype(np.int64)))
    return Epoch(b.keys, b.types, b.txn_begin[:(int(n[-1]) + 2) if n.size else 1].copy())


def pad_tail(b, tpr):
    """`b` with empty txns appended up to tpr txns (what dvcc.sequence needs
    to give every origin its tpr slots)"""
    return Epoch(b.keys, b.types, np.concatenate([b.txn_begin, np.full(tpr - b.n_txn, b.txn_begin[-1], np.uint32)]))


# ---- family 9: Ragged ladder(slots, stride, row_of).  `slots` lists the
# epoch's sequence slots: EMPTY (a txn without accesses), a pad count p >= 0 (a
# ladder txn), or ONE (a single private access).  The k-th ladder txn is
# [W row_of(k), W row_of(k + 1)] followed by p accesses of private rows, 2 + p
# <= kMaxPos; a private row is priv0 + stride * i for the epoch's i-th private
# access (priv0: the first multiple of stride past the ladder's rows), used
# once in the whole epoch, a write when i % 3 == 0 and a read otherwise.
# NO_WAIT / WAIT_DIE / OCC: private rows never conflict and no row repeats
# inside a txn (no H9), so the ladder decides as family 1 -- the k-th ladder
# txn commits iff k is even -- and empty and ONE txns commit.  CALVIN: all
# commit.  Under `row % world` ownership row_of and stride place the rows
# (ownership()).
EMPTY, ONE = None, -1


def ragged_ladder(slots, stride, row_of):
    kmax = structural_constants()["kMaxPos"]
    slots = list(slots)
    lens = np.array([0 if s is EMPTY else 1 if s == ONE else 2 + s for s in slots], np.int64)
    lad = np.array([s is not EMPTY and s != ONE for s in slots], bool)
    assert lens.max(initial=0) <= kmax and (lens[lad] >= 2).all()
    L = int(lad.sum())
    k = np.arange(L, dtype=np.int64)
    tb = np.zeros(len(slots) + 1, np.int64)
    tb[1:] = np.cumsum(lens)
    n = int(tb[-1])
    keys = np.zeros(n, np.int64)
    types = np.zeros(n, np.uint8)
    priv = np.ones(n, bool)
    a = tb[:-1][lad]  # the ladder txns' first accesses
    ladder_rows = np.asarray(row_of(np.arange(L + 1, dtype=np.int64)), np.int64)
    assert L == 0 or (np.diff(ladder_rows) > 0).all()
    keys[a], keys[a + 1] = ladder_rows[:-1], ladder_rows[1:]
    types[a] = types[a + 1] = WR
    priv[a] = priv[a + 1] = False
    i = np.arange(int(priv.sum()), dtype=np.int64)
    priv0 = (int(ladder_rows[-1]) // stride + 1) * stride
    keys[priv] = priv0 + stride * i
    types[priv] = (i % 3 == 0).astype(np.uint8)
    e = _mk(lens, keys, types)
    c = _ones(len(slots))
    c[lad] = k % 2 == 0
    exp = {cc: c.copy() for cc in LOCKING + ("OCC",)}
    exp["CALVIN"] = _ones(len(slots))
    return Case(e, priv0 + stride * len(i) + 1, exp)


OWNERSHIPS = ("spread", "part0", "skip_last")


def ownership(kind, world):
    """(row_of, stride) of a ragged ladder under `row % world` ownership:
    spread     ladder row k, private rows consecutive: every partition alike
    part0      every row a multiple of world: partition 0 owns everything
    skip_last  ladder rows on partitions 0 .. world - 2 in turn, private rows
               on partition 0: partition world - 1 owns nothing that is used"""
    if kind == "spread":
        return (lambda k: k), 1
    if kind == "part0":
        return (lambda k: world * k), world
    assert kind == "skip_last" and world >= 2
    return (lambda k: k + k // (world - 1)), world


# ---- the shapes: per-origin slot lists, laid out as the global epoch in
# either order so that its cut (contiguous_chunks for origin-major,
# strided_chunks for position-major, each batch then trim_tail'ed) hands every
# origin exactly its list
def arrange(per_origin, order, tpr=None):
    world = len(per_origin)
    tpr = tpr or max(1, max(len(s) for s in per_origin))
    grid = [list(s) + [EMPTY] * (tpr - len(s)) for s in per_origin]
    if order == "position":
        return [grid[q][j] for j in range(tpr) for q in range(world)]
    assert order == "origin"
    return [grid[q][j] for q in range(world) for j in range(tpr)]


def cut(e, world, order):
    """the origins' batches of global epoch `e` (trailing empty txns dropped)
    and txns_per_rank"""
    parts, tpr = strided_chunks(e, world) if order == "position" else contiguous_chunks(e, world)
    return [trim_tail(p) for p in parts], tpr


def _fill(total, unit):
    """pad counts of ladder txns of `unit` accesses holding `total` accesses
    in all, the last txn sized to land the total"""
    kmax = structural_constants()["kMaxPos"]
    assert 2 <= unit < kmax and (total == 0 or total >= 2)
    lens = [unit] * (total // unit)
    rem = total - unit * len(lens)
    if rem >= 2 or (rem and not lens):
        lens.append(rem)
    elif rem:
        lens[-1] += 1
    return [n - 2 for n in lens]


def _spread(total, n):
    """pad counts of n ladder txns holding `total` accesses as evenly as it goes"""
    kmax = structural_constants()["kMaxPos"]
    lens = np.full(n, total // n)
    lens[:total % n] += 1
    assert lens.min() >= 2 and lens.max() <= kmax
    return [int(x) - 2 for x in lens]


def _segment(total):
    """one origin's batch of `total` accesses; where it spans more than a tile
    of kXTile, a txn of kMaxPos accesses sits across the first tile edge"""
    K = structural_constants()
    X, M = K["kXTile"], K["kMaxPos"]
    if total < X + M:
        return _fill(total, 31)
    return _fill(X - M // 2, 31) + [M - 2] + _fill(total - X - M // 2, 31)


def segment_sizes():
    X = structural_constants()["kXTile"]
    return [X - 1, X, X + 1, 2 * X + 1]


def segment_edge_group(world, order, own="spread"):
    """Segment edges: a group's `world` epochs.  In epoch e one origin has no
    accesses at all (no txns: it stands first, in the middle, last, in turn
    over the epochs) and the others hold kXTile - 1, kXTile, kXTile + 1 and
    2 * kXTile + 1 accesses in turn -- what k_group_txn_count,
    k_group_txn_ids and k_il_move tile.  Returns (cases, txns_per_rank)."""
    sizes = segment_sizes()
    zero_at = [0, world // 2, world - 1]
    per_epoch, i = [], 0
    for e in range(world):
        per = []
        for q in range(world):
            if q == zero_at[e % 3]:
                per.append([])
            else:
                per.append(_segment(sizes[i % len(sizes)]))
                i += 1
        per_epoch.append(per)
    tpr = max(len(s) for per in per_epoch for s in per)
    row_of, stride = ownership(own, world)
    return [ragged_ladder(arrange(per, order, tpr), stride, row_of) for per in per_epoch], tpr


MOVE_KINDS = ("search", "exact", "over", "empties", "small")


def _move_tile(kind, nj):
    """nj txns of one k_il_move_tb tile holding: `small` 2 accesses each;
    `exact` kIlOwn accesses; `over` kIlOwn + 1; `search` an empty txn and then
    three of kMaxPos accesses, over and over (3 * kIlOwn at nj = kIlTxns:
    the binary search, with equal starts before every long txn); `empties`
    nothing"""
    K = structural_constants()
    if kind == "empties":
        return [EMPTY] * nj
    if kind == "small":
        return [0] * nj
    if kind == "search":
        return [EMPTY if j % 4 == 0 else K["kMaxPos"] - 2 for j in range(nj)]
    return _spread(K["kIlOwn"] + (kind == "over"), nj)


def move_tile_group(world, tpr, order="position", own="spread", first=0):
    """Move tiles: a group's `world` epochs of `tpr` txns per origin.  Every
    origin's batch is made of tiles of kIlTxns txns; the tiles of at least
    kIlTxns - 1 txns take MOVE_KINDS in turn (from `first`) over the group,
    a shorter last tile is `small`.  Returns (cases, txns_per_rank)."""
    T = structural_constants()["kIlTxns"]
    row_of, stride = ownership(own, world)
    cases, i = [], first
    for e in range(world):
        per = []
        for q in range(world):
            slots = []
            for j0 in range(0, tpr, T):
                nj = min(T, tpr - j0)
                if nj >= T - 1:
                    slots += _move_tile(MOVE_KINDS[i % len(MOVE_KINDS)], nj)
                    i += 1
                else:
                    slots += _move_tile("small", nj)
            per.append(slots)
        cases.append(ragged_ladder(arrange(per, order, tpr), stride, row_of))
    return cases, tpr


def wave_mix(world, own="spread", shift=0):
    """Wave mix: runs of 64 consecutive sequence slots (what one wave of the
    route's txn walk takes) mixing 0-, 1-, 2- and kMaxPos-access txns in a
    pattern of period 7, then 63 empty txns beside one of kMaxPos, then 64 of
    kMaxPos, then slots up to a multiple of `world`.  `shift` moves the
    pattern (a group's epochs differ)."""
    M = structural_constants()["kMaxPos"]
    pat = [EMPTY, M - 2, ONE, 0, EMPTY, 0, M - 2]
    slots = [pat[(i + shift) % len(pat)] for i in range(64 * 4)]
    slots += [EMPTY] * (63 - shift % 63) + [M - 2] + [EMPTY] * (shift % 63)
    slots += [M - 2] * 64
    tail = [0, ONE, M - 2]
    slots += [tail[i % 3] for i in range(-len(slots) % world)]
    row_of, stride = ownership(own, world)
    return ragged_ladder(slots, stride, row_of)
