"""Closed-loop refill, tracker and back-off at multi-chunk epoch sizes (a plain
module, shared by test_loop_cases_cpu.py and test_loop_cases_gpu.py).

The epoch sizes are derived from the constants of dvcc_carry.hip, read from
the source: with T = kCarryTpb txns a carry block and the one-workgroup scans
(k_carry_scan, k_bo_scan) taking per = ceil(nb / T) block counts a thread --
one count, 2 .. kR in registers, more than kR in a loop -- SIZES names the
smallest epochs that sit on each edge.

The hot-row pool.  Row 0 is the hot row H.  Pool txn i begins with a write: of
H when i is an H-writer, else of its own row 1 + i.  The rest of the txn is
len_i - 1 accesses, read, write, read .., of private rows 1 + P + 2 i + j that
no other txn touches.  An H-writer has at least one access; another txn may
have none, and then commits.

Commit formula.  Under NO_WAIT, WAIT_DIE and OCC alike, for any epoch of
distinct pool txns in any order: the first H-writer in sequence order takes H
(locks it / enters the validation history as its writer) and commits, every
later H-writer meets it and aborts, and no other txn shares a row with anyone:

    a txn commits iff it is not an H-writer, or it is the first H-writer of
    the epoch in sequence order.                                 (formula())

Every expected commit byte below comes from formula(); the oracle is asserted
equal to it for every epoch ("oracle off the formula"), and the models are
driven by it.

Which txns are H-writers runs by carry block of the pool, b = i // T, with a
period of 5 blocks (coprime to every per above): no H-writer / all T / all but
txn 7 of the block / only the block's last txn / every third txn.  On top of
that blocks [nb // 3, nb // 3 + 2 per) hold no H-writer and blocks
[2 nb // 3, 2 nb // 3 + 2 per) nothing else, nb = ceil(n_txn / T): either
stretch covers a whole scan chunk, whose counts then sum to 0 and to per T.

Seeded rings ("a ring the caller filled", include/dvcc.h): before a loop that
starts at tracker epoch E0 = 16, slot E0 % D holds c entries -- distinct
H-writers from the top of the pool, which the loop never draws, born before
E0, with the abort counts seed_aborts() prescribes by position.  Closed form
of the seeded epoch (c <= n_txn): the c released entries come first, in slot
order, then the fresh txns; every H-writer but the first -- the entry at
position 0 -- aborts; with ab the abort counts of the aborted txns in order
and cls = min(ab, log2 D), slot (E0 + 2^cls) % D then holds exactly the
aborted txns of class cls, in order (np.flatnonzero(cls == c): a stable
partition), each with the count min(ab + 1, 255).      (seeded_closed_form())
"""
import os
import re

import numpy as np

import _oracle as O
import dvcc
from dvcc import Epoch

ORACLE_CC = {dvcc.NO_WAIT: O.NO_WAIT, dvcc.WAIT_DIE: O.WAIT_DIE, dvcc.OCC: O.OCC}
E0 = 16  # the seeded loops' first tracker epoch

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva-plus_amd", "csrc")


def _src(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _const(text, name):
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)" % name, text).group(1))


def _body(text, kernel):
    """the text of one kernel: from its name to the next __global__"""
    at = re.search(r"void\s+%s\s*\(" % kernel, text).start()
    end = text.find("__global__", at)
    return text[at:end if end > 0 else len(text)]


def _cap(text, var):
    """the grid cap of a launch line `var > N ? N : var`"""
    m = re.search(r"%s\s*>\s*(\d+)\s*\?\s*(\d+)\s*:\s*%s\b" % (var, var), text)
    assert m and m.group(1) == m.group(2), var
    return int(m.group(1))


def constants():
    """kBlock / kCarryTpb, the two scans' kR, the tracker's and the back-off's
    constants and the three grid caps, from csrc/"""
    carry, internal = _src("dvcc_carry.hip"), _src("dvcc_internal.h")
    assert re.search(r"constexpr\s+uint32_t\s+kCarryTpb\s*=\s*kBlock\s*;", carry)
    kr = [_const(_body(carry, k), "kR") for k in ("k_carry_scan", "k_bo_scan")]
    assert kr[0] == kr[1], "k_carry_scan and k_bo_scan chunk alike"
    for k in ("k_carry_scan", "k_bo_scan"):
        assert re.search(r"if\s*\(\s*per\s*<=\s*kR\s*\)", _body(carry, k)), k
    refill = _body(carry, "launch_refill")
    backoff = carry[carry.index("static void launch_refill_backoff(hipStream_t s, const RefillReq &q) {"):]
    assert re.search(r"k_track_fresh,\s*gf\s*<\s*1\s*\?\s*1\s*:", refill) and "k_refill_fresh" in refill
    assert re.search(r"k_bo_spill,\s*gs\s*<\s*1\s*\?\s*1\s*:", backoff)
    return dict(
        kBlock=_const(internal, "kBlock"),
        kCarryTpb=_const(internal, "kBlock"),
        kR=kr[0],
        kTrackSlots=_const(internal, "kTrackSlots"),
        kTrackPer=_const(carry, "kTrackPer"),
        kTrackBins=_const(internal, "kTrackBins"),
        kBoClasses=_const(internal, "kBoClasses"),
        track_fresh_cap=_cap(refill, "gf"),
        refill_fresh_cap=_cap(refill, "g"),
        bo_spill_cap=_cap(backoff, "gs"),
    )


def sizes(k=None):
    k = k or constants()
    T, kR = k["kCarryTpb"], k["kR"]
    return dict(full_1=T * T, per_2=T * T + 1, per_kR=kR * T * T, per_loop=(kR * T + 2) * T - (T - 1))


def n_blocks(n, k):
    return (n + k["kCarryTpb"] - 1) // k["kCarryTpb"]


def per_of(n, k):
    """block counts a thread of the one-workgroup scans"""
    return (n_blocks(n, k) + k["kBlock"] - 1) // k["kBlock"]


def scan_path(n, k):
    p = per_of(n, k)
    return "one" if p == 1 else ("registers" if p <= k["kR"] else "loop")


def thread_chunks(n, k):
    """(first thread whose chunk nb cuts short or None, first thread with no
    count at all or None) of the scans' kBlock threads"""
    nb, per = n_blocks(n, k), per_of(n, k)
    held = np.clip(nb - np.arange(k["kBlock"], dtype=np.int64) * per, 0, per)
    short = np.flatnonzero((held > 0) & (held < per))
    none = np.flatnonzero(held == 0)
    return (int(short[0]) if len(short) else None, int(none[0]) if len(none) else None)


def track_groups(n, k):
    """workgroups of k_track_carry / k_bo_park: a wave a carry block"""
    wpb = k["kBlock"] // 64
    return (n_blocks(n, k) + wpb - 1) // wpb


def grid_passes(items, cap, k):
    """grid-stride passes of a kernel over `items` under a cap of `cap` workgroups"""
    per_pass = min(max(1, (items + k["kBlock"] - 1) // k["kBlock"]), cap) * k["kBlock"]
    return (items + per_pass - 1) // per_pass


# ---- the hot-row pool ---------------------------------------------------------
class HotPool:
    """epoch: the pool's txns (dvcc.Epoch); hw: which are H-writers; rows: the
    table's size"""

    def __init__(self, P, n_txn, lens, k=None):
        k = k or constants()
        T = k["kCarryTpb"]
        nb, per = n_blocks(n_txn, k), per_of(n_txn, k)
        i = np.arange(P, dtype=np.int64)
        b, r, kind = i // T, i % T, (i // T) % 5
        hw = (kind == 1) | ((kind == 2) & (r != 7)) | ((kind == 3) & (r == T - 1)) | ((kind == 4) & (r % 3 == 0))
        self.zero_at, self.full_at = nb // 3, 2 * nb // 3
        assert self.zero_at + 2 * per <= self.full_at and self.full_at + 2 * per <= nb - 1
        hw[(b >= self.zero_at) & (b < self.zero_at + 2 * per)] = False
        hw[(b >= self.full_at) & (b < self.full_at + 2 * per)] = True
        if lens == "mod4":
            ln = i % 4
            ln[0] = 1
            ln[hw] = np.maximum(ln[hw], 1)
        else:
            assert lens == "one"
            ln = np.ones(P, np.int64)
        tb = np.zeros(P + 1, np.int64)
        tb[1:] = np.cumsum(ln)
        txn = np.repeat(i, ln)
        j = np.arange(int(tb[-1]), dtype=np.int64) - tb[txn]
        keys = np.where(j == 0, np.where(hw[txn], 0, 1 + txn), 1 + P + 2 * txn + (j - 1))
        types = ((j & 1) == 0).astype(np.uint8)  # write, read, write
        self.P, self.n_txn, self.hw, self.lens = P, n_txn, hw, ln
        self.rows = 1 + P + (2 * P if lens == "mod4" else 0)
        self.epoch = Epoch(keys.astype(np.uint64), types, tb.astype(np.uint32))
        assert int(keys.max()) < self.rows < 1 << 31 and (ln[hw] >= 1).all()


_cache = {}


def pool(name, P=None, lens=None):
    """the pool of the size `name` (computed once, read-only afterwards): P
    defaults to four epochs, lens to "mod4" at the 65k sizes and "one" above"""
    n = sizes()[name]
    P = P if P is not None else (6 * n if n < 1 << 17 else 3 * n)
    lens = lens or ("mod4" if n < 1 << 17 else "one")
    key = ("pool", name, P, lens)
    if key not in _cache:
        _cache[key] = HotPool(P, n, lens)
    return _cache[key]


def formula(hw):
    """the commit bytes of an epoch whose txn t is an H-writer iff hw[t]"""
    c = np.ones(len(hw), np.uint8)
    c[np.flatnonzero(hw)[1:]] = 0
    return c


def epoch_of(p, src):
    """the epoch whose txn t holds the accesses of pool txn src[t]"""
    tb = p.epoch.txn_begin.astype(np.int64)
    src = np.asarray(src, np.int64)
    lens = tb[src + 1] - tb[src]
    ntb = np.zeros(len(src) + 1, np.int64)
    ntb[1:] = np.cumsum(lens)
    idx = np.repeat(tb[src] - ntb[:-1], lens) + np.arange(int(ntb[-1]), dtype=np.int64)
    return Epoch(p.epoch.keys[idx], p.epoch.types[idx], ntb.astype(np.uint32))


def carried_form(p, src, cap):
    """closed form of dv_epoch_carry behind the epoch of pool txns src: the
    H-writers but the first, in order, at most cap -- (their src, the epoch)"""
    ab = np.asarray(src)[np.flatnonzero(p.hw[src])[1:]][:cap]
    return ab, epoch_of(p, ab)


def decide(cc, p, tab, f0, src):
    """one epoch of pool txns src through the oracle, held to the formula:
    (commit bytes, the oracle's stats, the host epoch)"""
    assert len(np.unique(src)) == len(src), "a pool txn twice in one epoch"
    host = epoch_of(p, src)
    c = formula(p.hw[src])
    c_or, _, st = O.epoch_run(ORACLE_CC[cc], tab.ix, f0, host.n_txn, host.txn_begin, host.keys, host.types)
    assert np.array_equal(c_or[:host.n_txn], c), "oracle off the formula"
    assert st.committed == int(c.sum())
    return c, st, host


def run_model(cc, p, model, n_epochs, lanes=1):
    """n_epochs epochs of `model` (TrackModel, BackoffModel after build(), or
    the lanes model after start()) over the pool, each decided by the formula
    and the oracle: (per epoch (commit, stats, host epoch), the epochs left by
    number, the final table)"""
    tab = O.YcsbTable(p.rows)
    f0 = tab.f0.copy()

    def ids(e):
        if hasattr(model, "eps"):
            return model.eps[e][0]
        if hasattr(model, "ids"):
            return model.ids[e][0]
        assert e == model.k
        return model.ep[0]

    out = []
    for _ in range(n_epochs):
        c, st, host = decide(cc, p, tab, f0, ids(model.k))
        out.append((c, st, host))
        model.epoch(c)
    left = {model.k + ln: epoch_of(p, ids(model.k + ln)) for ln in range(lanes)}
    return out, left, f0


# ---- seeded rings -------------------------------------------------------------
def seed_aborts(c, T, head):
    """the abort counts of c seeded entries by position: carry block 0 mixed,
    then whole blocks of 0, of 2, of 3 and of 4 (one delay class each at
    D = 16: the low and the top field of c012, the low and the next field of
    c34), a block cycling 0, 1, 2, 3, 4 (a lane's four txns in four classes),
    a block of 253, 254, 255, 255, .., and the cycle again behind it; the
    entry at position 0 -- the seeded epoch's commit -- has `head`"""
    pos = np.arange(c, dtype=np.int64)
    b = pos // T
    ab = pos % 5
    ab[b == 0] = (pos[b == 0] * 7) % 6
    for blk, v in ((1, 0), (2, 2), (3, 3), (4, 4)):
        ab[b == blk] = v
    ab[b == 6] = np.minimum(253 + pos[b == 6] % T, 255)
    ab[0] = head
    return ab


def seed_entries(p, c, head, k=None):
    """(src, born, aborts) of c entries: the last c H-writers of the pool"""
    k = k or constants()
    src = np.flatnonzero(p.hw)[::-1][:c].copy()
    assert len(src) == c
    return src, E0 - 1 - (np.arange(c, dtype=np.int64) % 3), seed_aborts(c, k["kCarryTpb"], head)


def seed_model(model, entries):
    """the entries into slot E0 % D of a BackoffModel, before build()"""
    assert model.k == E0 and all(len(s[0]) == 0 for s in model.slots)
    model.slots[E0 % model.D] = tuple(np.asarray(a, np.int64).copy() for a in entries)
    model.fullest = max(model.fullest, len(entries[0]))
    return model


def seeded_closed_form(p, entries, fresh_src, D):
    """the seeded epoch (c <= n_txn released entries, then fresh_src) by the
    closed form: its commit bytes and, per slot that takes a class, (src,
    born, stored count) of what the park appends"""
    src = np.concatenate([entries[0], fresh_src])
    born = np.concatenate([entries[1], np.full(len(fresh_src), E0, np.int64)])
    ab = np.concatenate([entries[2], np.zeros(len(fresh_src), np.int64)])
    c = formula(p.hw[src])
    assert c[0] == 1 and p.hw[src[0]]
    lgD = D.bit_length() - 1
    dead = c == 0
    cls = np.minimum(ab[dead], lgD)
    parked = {}
    for q in range(lgD + 1):
        at = np.flatnonzero(cls == q)
        parked[(E0 + (1 << q)) % D] = (src[dead][at], born[dead][at], np.minimum(ab[dead][at] + 1, 255))
    return c, parked
