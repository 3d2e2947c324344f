"""Closed-form index tables (a plain module, shared by
test_index_cases_cpu.py and test_index_cases_gpu.py).

Every case is one table whose key -> local row map is known here by
construction: `where`, a Python dict built from the insertion order alone with
exact Python ints (the last insertion of a key wins, BucketHeader::insert_item
prepends a known key's item and read_item returns the head).  It is never
taken from the oracle or the engine; both are held to it.

A key of bucket b is written (q * nb + b) * P + lo: q the quotient the bucket
function drops, lo the residue (P = 1, lo = 0 under HASH_MOD).  The families:
  D1  dense, one partition (load_ycsb_partition)
  DP  dense partitions, part_cnt > 1; part_id kTagWide - 1 = 254 is the last
      with a narrow home tag, from kTagWide on the home tag is the wide
      sentinel and the map is no longer dense
  IM  implicit-row direct maps: load_table with one key per bucket in bucket
      order; quotients at every edge of the one-byte key tag
  EN  the same keys loaded in shuffled order: one {key, row} entry per bucket
  CH  chained tables: chains of 0, 1, 2, 64, 65 and 3,000 entries, and an
      empty table
  RP  a chained table with keys inserted two and three times
"""
import os
import re
from dataclasses import dataclass, field

import numpy as np

from dvcc import Epoch

CCS = ("NO_WAIT", "WAIT_DIE", "OCC", "CALVIN")
RD, WR = 0, 1
HASH_YCSB, HASH_MOD = 0, 1  # DV_HASH_* (include/dvcc.h)
U64 = 1 << 64

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva-plus_amd", "csrc")


def _src(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _const(text, name):
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)" % name, text).group(1))


def structural_constants():
    """kTagWide, kMaxTables, kPV, kBlock, kTile and kProbeHistTiles, from csrc/"""
    internal, kernels, math = _src("dvcc_internal.h"), _src("dvcc_kernels.hip"), _src("dvcc_index_math.h")
    assert re.search(r"constexpr\s+int\s+kTile\s*=\s*kBlock\s*\*\s*kIPT\s*;", internal)
    return dict(kTagWide=_const(math, "kTagWide"), kMaxTables=_const(internal, "kMaxTables"),
                kPV=_const(kernels, "kPV"), kBlock=_const(internal, "kBlock"),
                kTile=_const(internal, "kBlock") * _const(internal, "kIPT"),
                kProbeHistTiles=_const(internal, "kProbeHistTiles"))


K = structural_constants()
W = K["kTagWide"]


@dataclass
class IndexCase:
    name: str
    family: str
    form: str                    # "ycsb": load_ycsb_partition(rows); "table": create_table + load_table
    part_cnt: int = 1
    part_id: int = 0
    rows: int = 0                # rows of the table (its capacity; an empty table keeps one unused row)
    nbuckets: int = 0
    hash_kind: int = HASH_YCSB
    keys: list = field(default_factory=list)     # "table": the insertion order, row i = keys[i]
    f0: np.ndarray = None                        # the initial column [rows]
    where: dict = field(default_factory=dict)    # key -> local row
    present: list = field(default_factory=list)  # (label, key)
    missing: list = field(default_factory=list)  # (label, key)
    pairs: list = field(default_factory=list)    # (key, other key of the same bucket)

    @property
    def n(self):
        return len(self.keys) if self.form == "table" else self.rows

    def bucket(self, key):
        return (key // self.part_cnt) % self.nbuckets if self.hash_kind == HASH_YCSB else key % self.nbuckets

    def present_keys(self):
        out = []
        for _, k in self.present:
            if k not in out:
                out.append(k)
        return out


def f0_of_rows(n):
    """a distinct non-zero 64-bit value per row (an odd multiplier permutes the words)"""
    return ((np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))).astype(np.uint64)


def ycsb_f0(key):
    """a YCSB row's first field: "hello\\0", then bytes 6..7 of its key (ycsb_wl.cpp:173-186)"""
    return (key & 0xFFFF000000000000) | int.from_bytes(b"hello\0", "little")


def _key(nb, P, q, b, lo):
    return (q * nb + b) * P + lo


def _qmax(nb, P, b, lo):
    """the largest quotient that keeps bucket b's key of residue lo below 2^64"""
    q = ((U64 - 1 - lo) // P - b) // nb
    assert _key(nb, P, q, b, lo) < U64 <= _key(nb, P, q + 1, b, lo)
    return q


def _finish(c):
    assert len(c.missing) <= 64, (c.name, len(c.missing))
    for lab, k in c.missing:
        assert 0 <= k < U64 and k not in c.where, (c.name, lab, k)
    for lab, k in c.present:
        assert k in c.where, (c.name, lab, k)
    assert len({lab for lab, _ in c.present}) == len(c.present)
    assert len({lab for lab, _ in c.missing}) == len(c.missing)
    if c.form == "table":
        assert len(set(c.f0[:c.n].tolist())) == c.n and (c.f0[:c.n] != 0).all()
    return c


# ---- D1
def dense_one(rows):
    c = IndexCase(f"D1_{rows}", "D1", "ycsb", rows=rows, nbuckets=rows)
    c.where = {k: k for k in range(rows)}
    c.f0 = np.array([ycsb_f0(k) for k in range(rows)], np.uint64)
    c.present = [("first", 0), ("last", rows - 1)]
    c.missing = [("rows", rows), ("2^31", 1 << 31), ("2^63", 1 << 63), ("2^64-1", U64 - 1)]
    return _finish(c)


# ---- DP
DP_PARTS = ((3, 0), (3, 2), (7, 6), (300, 0), (300, 253), (300, 254), (300, 299))


def dense_part(P, part, rows=1000):
    c = IndexCase(f"DP_{P}_{part}", "DP", "ycsb", part_cnt=P, part_id=part, rows=rows, nbuckets=rows)
    c.where = {r * P + part: r for r in range(rows)}
    c.f0 = np.array([ycsb_f0(r * P + part) for r in range(rows)], np.uint64)
    c.present = [(f"r={r}", r * P + part) for r in (0, 1, rows - 1)]
    r = 1
    c.missing = [("residue+1", r * P + (part + 1) % P), ("residue-1", r * P + (part - 1) % P),
                 ("q=1", _key(rows, P, 1, r, part)), ("q=1,r=0", _key(rows, P, 1, 0, part)),
                 ("q=1,r=last", _key(rows, P, 1, rows - 1, part))]
    c.missing += [(f"q={q}", _key(rows, P, q, r, part)) for q in (W - 1, W, W + 1)]
    c.missing += [("q=max", _key(rows, P, _qmax(rows, P, r, part), r, part))]
    return _finish(c)


# ---- IM / EN
QS = ("0", "1", "W-2", "W-1", "W", "W+1", "2^40", "max")


def _quot(name, nb, P, b, lo):
    return {"0": 0, "1": 1, "W-2": W - 2, "W-1": W - 1, "W": W, "W+1": W + 1, "2^40": 1 << 40,
            "max": _qmax(nb, P, b, lo)}[name]


def direct_map(hash_kind, nb, variant="cycle", shuffled=False):
    """one key per bucket.  cycle: bucket b's quotient is QS[b % 8]; home90:
    nine buckets of ten hold quotient 1 and residue 0 (the home tag), the tenth cycles;
    flat: quotient b % 20, no tag above a 5 % share.  The bucket 2^64 - 1
    belongs in holds it."""
    P = 3 if hash_kind == HASH_YCSB else 1
    fam = "EN" if shuffled else "IM"
    c = IndexCase(f"{fam}_{'ycsb3' if P > 1 else 'mod'}_{nb}_{variant}", fam, "table", part_cnt=P, rows=nb,
                  nbuckets=nb, hash_kind=hash_kind)
    top = U64 - 1
    b_top, lo_top = c.bucket(top), top % P
    qname, keys = [], []
    for b in range(nb):
        lo = b % P
        if variant == "cycle":
            qn = QS[b % 8]
        elif variant == "home90":
            qn = QS[(b // 10) % 8] if b % 10 == 9 else "1"
            if qn == "1":
                lo = 0  # (one residue: the home rows share the tag P, under either hash)
        else:
            assert variant == "flat"
            qn = None
        if b == b_top:
            qn, lo = "max", lo_top
        q = b % 20 if qn is None else _quot(qn, nb, P, b, lo)
        qname.append(qn or f"{q}")
        keys.append(_key(nb, P, q, b, lo))
    assert keys[b_top] == top
    order = list(range(nb))
    if shuffled:
        order = np.random.default_rng(nb).permutation(nb).tolist()
        assert order != sorted(order)
    c.keys = [keys[b] for b in order]
    c.where = {k: i for i, k in enumerate(c.keys)}
    assert len(c.where) == nb
    c.f0 = f0_of_rows(nb)
    # the probed buckets: one of every quotient of the cycle, the bucket of 2^64 - 1 and the last one
    probed = sorted(set(list(range(min(nb, 8))) + [b_top, nb - 1]))
    for b in probed:
        k = keys[b]
        lo, q = k % P, k // P // nb
        c.present.append((f"b={b},q={qname[b]}", k))
        if _key(nb, P, q + 1, b, lo) < U64:
            c.missing.append((f"b={b},q={qname[b]}+1", _key(nb, P, q + 1, b, lo)))
        if q > 0:
            c.missing.append((f"b={b},q={qname[b]}-1", _key(nb, P, q - 1, b, lo)))
        for d in range(1, P):
            k2 = _key(nb, P, q, b, (lo + d) % P)
            if k2 < U64:
                c.missing.append((f"b={b},q={qname[b]},lo+{d}", k2))
    return _finish(c)


# ---- CH / RP
def chained(hash_kind, nb, lengths, name, repeats=False):
    """bucket b's chain has lengths[b] keys: quotients 0, 1, W-1, W, W+1, 2^40,
    the largest, then 2, 3, ...; inserted in a seeded shuffle over all
    buckets.  repeats: every chain of 3 keys or more has its second key
    inserted again after the third and its first key again after that and
    once more at the very end of the load (three insertions)."""
    P = 3 if hash_kind == HASH_YCSB else 1
    assert len(lengths) == nb
    fam = "RP" if repeats else "CH"
    c = IndexCase(name, fam, "table", part_cnt=P, nbuckets=nb, hash_kind=hash_kind)
    rng = np.random.default_rng(len(name) + nb)
    chains, unused = [], {}
    for b, n in enumerate(lengths):
        lo = b % P
        edges = [0, 1, W - 1, W, W + 1, 1 << 40, _qmax(nb, P, b, lo)]
        qs = edges[:n] + [q for q in range(2, 2 + n + 3) if q not in edges][:max(0, n - len(edges))]
        assert len(qs) == n == len(set(qs))
        chains.append([_key(nb, P, q, b, lo) for q in qs])
        unused[b] = _key(nb, P, max(2 + n, 300) + 7, b, lo)  # a quotient no chain uses
    # the insertion order: a shuffle of (bucket, position) that keeps each chain's own order
    slots = np.repeat(np.arange(nb), lengths)
    rng.shuffle(slots)
    at = [0] * nb
    late = []
    for b in slots.tolist():
        c.keys.append(chains[b][at[b]])
        at[b] += 1
        if repeats and at[b] == 3:
            c.keys.append(chains[b][1])   # second insertion of the chain's second key
        if repeats and at[b] == min(5, lengths[b]) and lengths[b] >= 3:
            c.keys.append(chains[b][0])   # second insertion of the chain's first key
            late.append(chains[b][0])
    c.keys += late                        # ... and its third
    if repeats:
        for i in range(1, len(c.keys)):
            assert c.keys[i] != c.keys[i - 1], "a repeated key next to itself"
    for i, k in enumerate(c.keys):
        c.where[k] = i                    # the newest insertion wins
    c.rows = max(1, len(c.keys))
    c.f0 = np.zeros(c.rows, np.uint64)    # (an empty table's one row is never loaded: zero)
    c.f0[:len(c.keys)] = f0_of_rows(len(c.keys))
    longest = int(np.argmax(lengths))
    for b, ch in enumerate(chains):
        if not ch:
            continue
        c.present.append((f"b={b},len={len(ch)},first", ch[0]))
        if len(ch) > 1:
            c.present.append((f"b={b},len={len(ch)},last", ch[-1]))
            if len(c.pairs) < 4:
                c.pairs.append((ch[0], ch[-1]))
        if repeats and len(ch) >= 3:
            c.present.append((f"b={b},len={len(ch)},second", ch[1]))
    if len(c.keys):
        c.missing.append(("longest chain's bucket", unused[longest]))
        k = chains[longest][-1]
        q, lo = k // P // nb, k % P
        c.missing.append(("last of the longest chain, q+1", _key(nb, P, q + 1, longest, lo)))
    empty = [b for b in range(nb) if lengths[b] == 0]
    for b in (empty[:1] + empty[-1:]) if len(empty) > 1 else empty:
        c.missing.append((f"empty bucket {b},q=0", _key(nb, P, 0, b, b % P)))
        c.missing.append((f"empty bucket {b},q=max", _key(nb, P, _qmax(nb, P, b, b % P), b, b % P)))
    if P > 1 and len(c.keys):
        k = chains[longest][0]
        c.missing.append(("other residue", k - k % P + (k % P + 1) % P))
    return _finish(c)


def _ch_lengths(nb):
    """first and last bucket empty; chains of 1, 2, 64, 65 and 3,000; the rest 0, 1, 2 in turn"""
    ln = [b % 3 for b in range(nb)]
    ln[0] = ln[nb - 1] = 0
    ln[1:6] = [1, 2, 64, 65, 3000]
    return ln


def _builders():
    cs = {}

    def add(fn, *a, **kw):
        cs[len(cs)] = (fn, a, kw)
    for rows in (33, 4096):
        add(dense_one, rows)
    for P, part in DP_PARTS:
        add(dense_part, P, part)
    for hk in (HASH_MOD, HASH_YCSB):
        for nb in (1, 33, 1021):
            add(direct_map, hk, nb)
        for nb in (33, 1021):
            add(direct_map, hk, nb, "home90")
            add(direct_map, hk, nb, "flat")
            add(direct_map, hk, nb, "cycle", shuffled=True)
        add(direct_map, hk, 1021, "home90", shuffled=True)
    add(chained, HASH_MOD, 97, _ch_lengths(97), "CH_mod_97")
    add(chained, HASH_YCSB, 97, _ch_lengths(97), "CH_ycsb3_97")
    add(chained, HASH_MOD, 1, [65], "CH_mod_1")
    add(chained, HASH_YCSB, 1, [64], "CH_ycsb3_1")
    add(chained, HASH_MOD, 97, [0] * 97, "CH_empty_97")
    add(chained, HASH_MOD, 97, _ch_lengths(97), "RP_mod_97", repeats=True)
    add(chained, HASH_YCSB, 1, [9], "RP_ycsb3_1", repeats=True)
    return cs


_BUILDERS = _builders()
_CASES = {}


def case_names():
    """every case's name (the cases themselves are built on first use)"""
    if not _CASES:
        for i, (fn, a, kw) in _BUILDERS.items():
            c = fn(*a, **kw)
            assert c.name not in _CASES
            _CASES[c.name] = c
    return list(_CASES)


def case(name):
    case_names()
    return _CASES[name]


# ---------------------------------------------------------------- the epochs
def _mk(txns, tables=None):
    """an Epoch of txns [[(key, type), ...], ...]"""
    tb = np.zeros(len(txns) + 1, np.uint32)
    tb[1:] = np.cumsum([len(t) for t in txns])
    keys = np.array([k for t in txns for k, _ in t], dtype=np.uint64)
    types = np.array([w for t in txns for _, w in t], dtype=np.uint8)
    return Epoch(keys, types, tb, tables=tables)


@dataclass
class EpochCase:
    epoch: Epoch
    expected: dict       # cc name -> uint8 [n_txn]
    written: dict        # cc name -> the keys written by committed txns


def read_epoch(c):
    """one txn per present key reading it, then one txn writing the first of
    them: the readers commit; the writer meets a committed read lock (NO_WAIT
    aborts it, WAIT_DIE's younger requester dies), under OCC earlier committed
    reads never invalidate and under CALVIN everything commits"""
    ks = c.present_keys()
    if not ks:
        return EpochCase(_mk([]), {cc: np.zeros(0, np.uint8) for cc in CCS}, {cc: [] for cc in CCS})
    e = _mk([[(k, RD)] for k in ks] + [[(ks[0], WR)]])
    exp, wr = {}, {}
    for cc in CCS:
        x = np.ones(len(ks) + 1, np.uint8)
        x[-1] = cc in ("OCC", "CALVIN")
        exp[cc], wr[cc] = x, [ks[0]] if x[-1] else []
    return EpochCase(e, exp, wr)


def write_epoch(c, seed=5):
    """one single-write txn per present key in a seeded permutation: distinct
    rows, so every txn commits under all four algorithms"""
    ks = c.present_keys()
    ks = [ks[i] for i in np.random.default_rng(seed).permutation(len(ks))]
    e = _mk([[(k, WR)] for k in ks])
    return EpochCase(e, {cc: np.ones(len(ks), np.uint8) for cc in CCS}, {cc: list(ks) for cc in CCS})


def pair_epoch(c):
    """per (k1, k2) of one bucket: [W k1], [W k2] -- different rows, both
    commit; an index that aliased them would abort the second.  Then [W k],
    [W k] on a key no pair uses: the second aborts under NO_WAIT, WAIT_DIE and
    OCC (the first holds its lock / wrote the row), CALVIN commits both."""
    txns, exp = [], []
    for k1, k2 in c.pairs:
        txns += [[(k1, WR)], [(k2, WR)]]
        exp += [(1, 1), (1, 1)]
    used = {k for p in c.pairs for k in p}
    same = [k for k in c.present_keys() if k not in used][:1]
    for k in same:
        txns += [[(k, WR)], [(k, WR)]]
        exp += [(1, 1), (0, 1)]
    e = _mk(txns)
    expd = {cc: np.array([x[cc == "CALVIN"] for x in exp], np.uint8) for cc in CCS}
    return EpochCase(e, expd, {cc: sorted(used) + same for cc in CCS})


def pad_epoch(c, probes, n_acc, wr=RD):
    """single-access txns reading `probes` in order, padded to n_acc accesses
    by txns reading an unrelated present key (the last present key that is no
    probe; a table of one key pads with it, an empty table not at all): read
    locks never conflict, every txn commits"""
    pad = [k for k in c.present_keys() if k not in probes] or c.present_keys()
    assert n_acc >= len(probes)
    return _mk([[(k, wr)] for k in probes] + ([[(pad[-1], RD)]] * (n_acc - len(probes)) if pad else []))


def column_after(c, written):
    """the initial column with zero exactly at where[key] of every written key"""
    f0 = c.f0.copy()
    for k in written:
        f0[c.where[k]] = 0
    return f0


def oracle_table(c):
    """the oracle's index over the case's insertions, in their order (an
    object with .ix; its rows' initial column is c.f0)"""
    import _oracle as O
    if c.form == "ycsb":
        return O.YcsbTable(c.rows, c.part_cnt, c.part_id)
    return O.MultiIndex(c.nbuckets, c.part_cnt, 1 if c.hash_kind == HASH_YCSB else 0,
                        [(k, i) for i, k in enumerate(c.keys)])


def oracle_read(t, key):
    """or_index_read on oracle_table(c): the row the oracle's index holds for
    `key` (a repeated key's newest), or None for a missing key (fatal in the
    reference, index_hash.cpp:225)"""
    import ctypes

    import _oracle as O
    row = ctypes.c_uint64()
    return row.value if O.lib().or_index_read(t.ix, key, ctypes.byref(row)) == 0 else None


def mix64(z):
    """the digests' mixer (splitmix64's finalizer, as oracle.c's or_mix64) over uint64 arrays"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def read_digest(values, txns, keys):
    """the committed-read digest: the sum over the committed reads of
    mix64(value ^ mix64(txn << 32 ^ key)), mod 2^64"""
    v, t, k = (np.asarray(x, np.uint64) for x in (values, txns, keys))
    with np.errstate(over="ignore"):
        return int(mix64(v ^ mix64((t << np.uint64(32)) ^ k)).sum(dtype=np.uint64))


def flat_epoch(c, n_acc, at=None, key=None, tables=None):
    """n_acc single-access read txns of one present key (the last), access
    `at` reading `key` instead: every txn commits, or the epoch is rejected
    when `key` is missing.  A table without keys has no such epoch but the
    one access."""
    ks = c.present_keys()
    keys = [ks[-1]] * n_acc if ks else [key]
    if at is not None and ks:
        keys[at] = key
    return _mk([[(k, RD)] for k in keys], tables=tables)


# ---------------------------------------------------------------- partitions of a replicated epoch
def rep_partition(P, part, home_q, nb=33):
    """Partition `part` of P as an implicit-row direct map that is not dense
    (load_table in bucket order, HASH_YCSB): bucket b holds (q_b * nb + b) * P
    + part with q_b = home_q, but the other of {0, 1} where b % 8 == 3 and
    kTagWide where b % 8 == 5.  A replicated epoch's key is its global row:
    only the rows of quotient 0 hold one (key b * P + part, local row b).
    home_q = 0: the home tag is the partition's own, an own key is decided by
    the home-tag bitmap; home_q = 1: it is another tag, own keys go by the
    key-tag byte and, where that is the wide sentinel, by the pkey word.
    present: rows of quotient 0; missing: the own keys of the other rows."""
    c = IndexCase(f"REP_{P}_{part}_home{home_q}", "REP", "table", part_cnt=P, part_id=part, rows=nb, nbuckets=nb,
                  hash_kind=HASH_YCSB)
    qs = [(1 - home_q) if b % 8 == 3 else W if b % 8 == 5 else home_q for b in range(nb)]
    c.keys = [_key(nb, P, q, b, part) for b, q in enumerate(qs)]
    c.where = {k: b for b, k in enumerate(c.keys)}
    c.f0 = f0_of_rows(nb) ^ np.uint64(part + 1)   # (distinct across the partitions too)
    zero = [b for b in range(nb) if qs[b] == 0]
    c.present = [(f"b={b}", b * P + part) for b in (zero[0], zero[len(zero) // 2], zero[-1])]
    for what, q in (("q=1", 1), ("q=W", W)):
        bs = [b for b in range(nb) if qs[b] == q]
        c.missing += [(f"own key of b={b}, which holds {what}", b * P + part) for b in (bs[0], bs[-1])]
    c.missing += [("past the rows", 2 * nb * P + part), ("2^32 + an own key", (1 << 32) + c.present[0][1]),
                  ("2^64 - 1 - (2^64 - 1 - part) % P", U64 - 1 - (U64 - 1 - part) % P)]
    return _finish(c)


def rep_group(world):
    """the partitions of a replicated group: home tag own, other, own"""
    return [rep_partition(world, p, p % 2) for p in range(world)]
