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
    the Bloom filter's bits, from csrc/."""
    rounds, internal, prefix = _src("dvcc_rounds.hip"), _src("dvcc_internal.h"), _src("dvcc_prefix.hip")
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
    )


# ---- family 1: Ladder(L).  T_k = [W k, W k+1], k < L.
# NO_WAIT / WAIT_DIE / OCC: T_0 commits, T_1 meets T_0's lock (write) on row 1
# and aborts, T_2 then finds row 2 free ... T_k commits iff k is even.
# CALVIN: all commit.  A dependency chain L deep: T_k's verdict needs T_{k-1}'s.
def ladder(L, empties=False):
    k = np.arange(L, dtype=np.int64)
    keys = np.stack([k, k + 1], 1).ravel()
    lens = np.full(L, 2)
    even = (k % 2 == 0).astype(np.uint8)
    if empties:  # family 8: an empty txn after every ladder txn (empties commit)
        lens = np.stack([lens, np.zeros(L, np.int64)], 1).ravel()
        even = np.stack([even, _ones(L)], 1).ravel()
    e = _mk(lens, keys, _ones(2 * L))
    exp = {cc: even.copy() for cc in LOCKING + ("OCC",)}
    exp["CALVIN"] = _ones(e.n_txn)
    # the aborted txns, in order and renumbered from 0: the odd ladder txns,
    # L // 2 of them with 2 accesses each; they touch disjoint rows (k, k+1
    # for odd k), so run as the next epoch all of them commit
    odd = k[1::2]
    carried = _mk(np.full(len(odd), 2), np.stack([odd, odd + 1], 1).ravel(), _ones(2 * len(odd)))
    return Case(e, L + 1, exp, carried=carried)


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
def carry_blocks(B):
    k = np.arange(B, dtype=np.int64)
    tail_n = 37
    ti = np.arange((tail_n + 1) // 2, dtype=np.int64)
    tl = np.zeros(tail_n, np.int64)
    tl[0::2] = 1
    lens = np.r_[np.zeros(B, np.int64), np.ones(3 * B, np.int64), tl]
    keys = np.r_[k, k, B + k, B + ti]
    e = _mk(lens, keys, _ones(len(keys)))
    c = np.r_[_ones(2 * B), np.zeros(B, np.uint8), _ones(B), (tl == 0).astype(np.uint8)]
    ck = np.r_[k, B + ti]
    carried = _mk(np.ones(len(ck), np.int64), ck, _ones(len(ck)))
    return Case(e, 2 * B + 8, {cc: c.copy() for cc in LOCKING + ("OCC",)}, carried=carried)


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
