"""k_kill's state reads (csrc/dvcc_prefix.hip): a step's accesses read one
word of the LDS array each -- the hot rows' bitmap words, the Bloom filter --
and the cold ones whose filter bit is set gather their bitmap word from L2,
each batch in flight at once, the next step's records behind the gathers.

Every case is a prefix-kill epoch forced small with set_prefix(K) on a table of
2^21 rows (two rows on every filter bit), built so that its commit bytes follow
from a formula: the K prefix txns touch rows of their own and all commit; a
later txn dies iff it touches a row a prefix txn wrote or (NO_WAIT / WAIT_DIE)
writes a row a prefix txn read; the later txns conflict with one another
nowhere.  The oracle is held to the formula, and the engine to the oracle bit
for bit: commit bytes, counts, read digest and the whole table -- plus the
survivors and their kept accesses (the skip bits) against the formula.

Each case runs through k_kill's three instantiations and both loops of the
dense one: 4-byte records (`recs`) and keys + types (`keys`) on the dense map,
a hashed index (`hashed`), and an epoch without boundaries (`acc_txn`).
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import _oracle as O
import adversarial as A
import dvcc
from dvcc import CCEngine, DeviceEpoch, Epoch

gpu = pytest.mark.gpu

CC = {"NO_WAIT": dvcc.NO_WAIT, "WAIT_DIE": dvcc.WAIT_DIE, "OCC": dvcc.OCC}
OCC_ID = {"NO_WAIT": O.NO_WAIT, "WAIT_DIE": O.WAIT_DIE, "OCC": O.OCC}
VARIANTS = ("recs", "keys", "hashed", "acc_txn")
ROWS = 1 << 21
HOT = A.structural_constants()["kHotRows"]
BLOOM_BITS = A.structural_constants()["kBloomBits"]
_PREFIX_SRC = A._src("dvcc_prefix.hip")
KILL_WORDS = A._define(_PREFIX_SRC, "DVCC_KILL_WORDS")
# bloom_bit(row) = (row * M) >> (32 - DVCC_BLOOM_LOG), the multiplier from the source
BLOOM_MUL = int(re.search(r"bloom_bit\(uint32_t row\)\s*\{\s*return \(row \* (0x[0-9A-Fa-f]+)u\)", _PREFIX_SRC).group(1), 16)
RD, WR = 0, 1
K_SMALL = 64


def bloom_bit(rows):
    shift = 32 - (BLOOM_BITS.bit_length() - 1)
    return ((np.asarray(rows, np.uint64) * np.uint64(BLOOM_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)


@functools.lru_cache(maxsize=None)
def colliders(n):
    """n pairs (A, B) of cold rows on one filter bit, in different bitmap
    words, every row and its neighbour (row ^ 1) distinct over the pairs"""
    rows = np.arange(HOT + 4096, ROWS, dtype=np.int64)
    h = bloom_bit(rows).astype(np.int64)
    order = np.argsort(h, kind="stable")
    hs, rs = h[order], rows[order]
    same = np.flatnonzero(hs[1:] == hs[:-1])
    out, used = [], set()
    for i in same[:: max(1, len(same) // (8 * n))]:
        a, b = int(rs[i]), int(rs[i + 1])
        cells = {a, a ^ 1, b, b ^ 1}
        if a >> 4 != b >> 4 and len(cells) == 4 and not (cells & used):
            out.append((a, b))
            used |= cells
            if len(out) == n:
                return tuple(out)
    raise AssertionError("not enough colliding rows")


class Case:
    """keys are rows (the dense map); a hashed table maps key 7 * row + 3 to row"""

    def __init__(self, rows, types, tb, k, m_wr, m_rd):
        self.rows, self.types, self.tb, self.k = rows.astype(np.uint64), types.astype(np.uint8), tb.astype(np.uint32), k
        self.n_txn, self.n_acc, self.a_acc = len(tb) - 1, int(tb[-1]), int(tb[k])
        self.m_wr, self.m_rd = m_wr, m_rd  # bool [ROWS]: written / only read by the prefix

    def facts(self, cc):
        """(commit bytes, survivors, their kept accesses) by the formula"""
        locking = cc != "OCC"
        r = self.rows.astype(np.int64)
        kill = self.m_wr[r] | (self.m_rd[r] & (self.types == WR) if locking else False)
        skip = self.m_rd[r] & (self.types == RD) if locking else np.zeros(self.n_acc, bool)
        kill[:self.a_acc] = False
        starts = self.tb[:-1].astype(np.int64)
        lens = np.diff(self.tb.astype(np.int64))
        # (an empty txn's reduceat slot holds its neighbour's value: masked by lens)
        killed = (np.add.reduceat(np.r_[kill, False].astype(np.int64), starts) > 0) & (lens > 0)
        commit = (~killed).astype(np.uint8)
        later = np.arange(self.n_txn) >= self.k
        kept = np.add.reduceat(np.r_[~skip, False].astype(np.int64), starts) * (lens > 0)
        surv = later & ~killed
        return commit, int(surv.sum()), int(kept[surv].sum())

    def epoch(self, hashed):
        keys = self.rows * np.uint64(7) + np.uint64(3) if hashed else self.rows
        return Epoch(np.ascontiguousarray(keys), self.types, self.tb)


def build(seed, n_later, hits, wt=(), rt=(), a_mod=0, n_mod=None, k=K_SMALL, reserved=(), mark_frac=0.0, later_len=10):
    """k prefix txns over rows of their own -- `wt` written, `rt` read, the
    rest filler -- with a_acc = a_mod (mod 64); n_later txns of about
    `later_len` accesses, n_acc = n_mod (mod 64) when given: reads of a shared
    pool of unmarked rows (40 % of them hot rows) and writes of rows used
    once.  hits: (j, lane, row, type) puts that access at index
    ((a_acc >> 6) + j) * 64 + lane; row -1 / -2 there stand for the very first
    and the very last later access.  mark_frac: that share of the later
    accesses, at random, touch a row the prefix marked (any access of a
    written row, reads of a read one).  `reserved` rows are kept out of every
    pool."""
    rng = np.random.default_rng(seed)
    special = np.array(sorted(set(wt) | set(rt) | set(reserved) | {r for h in hits for r in [h[2]] if r >= 0}), np.int64)
    free = rng.permutation(ROWS)
    free = free[~np.isin(free, special)]
    # the prefix: 5 accesses a txn and a_mod more, the targets first
    plens = np.full(k, 5)
    plens[:a_mod] += 1
    n_pre = int(plens.sum())
    assert n_pre % 64 == a_mod and len(wt) + len(rt) <= n_pre
    n_fill = n_pre - len(wt) - len(rt)
    fill, free = free[:n_fill], free[n_fill:]
    prow = np.r_[np.array(wt, np.int64), np.array(rt, np.int64), fill]
    ptyp = np.r_[np.full(len(wt), WR), np.full(len(rt), RD), rng.integers(0, 2, n_fill)].astype(np.uint8)
    mix = rng.permutation(n_pre)
    prow, ptyp = prow[mix], ptyp[mix]
    m_wr, m_rd = np.zeros(ROWS, bool), np.zeros(ROWS, bool)
    m_wr[prow[ptyp == WR]] = True
    m_rd[prow[ptyp == RD]] = True
    # the later txns
    llens = rng.integers(later_len - 2, later_len + 3, size=n_later)
    if n_mod is not None:
        llens[-1] += (n_mod - n_pre - int(llens.sum())) % 64
    n_lat = int(llens.sum())
    is_wr = rng.random(n_lat) < 0.25
    n_w = int(is_wr.sum())
    wpool, rpool = free[:n_w], free[n_w:]
    hot_pool, cold_pool = rpool[rpool < HOT], rpool[rpool >= HOT]
    assert len(hot_pool) > 1000 and len(cold_pool) > 1000
    pick_hot = rng.random(n_lat) < 0.4
    lrow = np.where(pick_hot, hot_pool[rng.integers(0, len(hot_pool), n_lat)],
                    cold_pool[rng.integers(0, len(cold_pool), n_lat)])
    lrow[is_wr] = wpool
    ltyp = is_wr.astype(np.uint8)
    if mark_frac:
        at = np.flatnonzero(rng.random(n_lat) < mark_frac)
        marked = prow[rng.integers(0, n_pre, len(at))]
        lrow[at] = marked
        ltyp[at] = np.where(m_wr[marked], rng.integers(0, 2, len(at)), RD)
    w0 = n_pre >> 6
    for j, lane, row, typ in hits:
        i = {-1: n_pre, -2: n_pre + n_lat - 1}[row] if row < 0 else ((w0 + j) << 6) + lane
        assert n_pre <= i < n_pre + n_lat, (j, lane, i)
        lrow[i - n_pre], ltyp[i - n_pre] = (wt[0] if row < 0 else row), typ
    tb = np.zeros(k + n_later + 1, np.int64)
    tb[1:] = np.cumsum(np.r_[plens, llens])
    case = Case(np.r_[prow, lrow], np.r_[ptyp, ltyp], tb, k, m_wr, m_rd)
    # what the formula rests on: a row the prefix only read is written by at
    # most one later access, and nothing touches it after that write
    lr, lt = case.rows[n_pre:].astype(np.int64), case.types[n_pre:]
    for r in np.unique(lr[(lt == WR) & m_rd[lr]]):
        where = np.flatnonzero(lr == r)
        assert (lt[where] == WR).sum() == 1 and lt[where[-1]] == WR, f"row {r}: written twice or touched after its write"
    return case


def step_hits(rows_types):
    """one hit in every word of a step at lanes 0, 31 and 63: word q of the
    step that begins 8 * (1 + 3 q + l) words after the first later word"""
    hits = []
    for q in range(KILL_WORDS):
        for li, lane in enumerate((0, 31, 63)):
            row, typ = rows_types[(3 * q + li) % len(rows_types)]
            hits.append((KILL_WORDS * (1 + 3 * q + li) + q, lane, row, typ))
    return hits


WT = (5, HOT - 2, HOT + 77, ROWS - 1)          # written by the prefix: hot, hot, cold, the last row
RT = (9, HOT - 3, HOT + 99, ROWS - 19)         # read by the prefix, read by later txns
RTW = tuple(HOT - 40 + 9 * i for i in range(8))  # read by the prefix, each written by one later txn (both sides of HOT)


@functools.lru_cache(maxsize=None)
def case_of(name):
    if name.startswith("boundary_"):
        # rows kHotRows - 1, kHotRows, kHotRows + 1 written (wr) or only read (rd)
        # by the prefix; later txns read each twice and then write it once
        edge = (HOT - 1, HOT, HOT + 1)
        hits = []
        for i, r in enumerate(edge):
            hits += [(3 + 2 * i, 7 + i, r, RD), (20 + 2 * i, 40 + i, r, RD), (60 + 2 * i, 13 + i, r, WR)]
        wr = name == "boundary_wr"
        return build(11, 1200, hits, wt=edge if wr else (), rt=() if wr else edge, a_mod=17)
    if name == "collide":
        # A0, A1 written by the prefix; B0, B1 on their filter bits and A0 ^ 1,
        # A1 ^ 1 in their bitmap words are touched by later txns alone: B0 and
        # A0 ^ 1 read three times, B1 and A1 ^ 1 written once
        (a0, b0), (a1, b1) = colliders(2)
        assert bloom_bit([a0, a1]).tolist() == bloom_bit([b0, b1]).tolist()
        hits = [(2, 3, a0, RD), (4, 60, a0, WR), (6, 33, a1, RD), (9, 1, a1, WR)]
        hits += [(11 + 5 * i, 9 * i, b0, RD) for i in range(3)] + [(12 + 5 * i, 11 * i, a0 ^ 1, RD) for i in range(3)]
        hits += [(30, 17, b1, WR), (33, 48, a1 ^ 1, WR)]
        return build(12, 1200, hits, wt=(a0, a1), a_mod=5)
    if name.startswith("pos_"):
        # a_acc = a_mod, n_acc = n_mod (mod 64); a hit in every word of a step at
        # lanes 0, 31 and 63, the first and the last later access hits too
        a_mod, n_mod = (int(x) for x in name[4:].split("_"))
        # (those on rows the prefix wrote: they kill under every algorithm);
        # between them reads of rows the prefix read -- skipped -- and one write
        # of each RTW row, which kills under NO_WAIT / WAIT_DIE
        hits = step_hits([(WT[0], RD), (WT[1], WR), (WT[2], RD), (WT[3], WR), (WT[2], WR), (WT[1], RD), (WT[3], RD)])
        hits += [(5 + 7 * i, (13 * i) % 64, RT[i % 4], RD) for i in range(16)]
        hits += [(3 + 11 * i, (37 * i + 5) % 64, r, WR) for i, r in enumerate(RTW)]
        assert len({(h[0], h[1]) for h in hits}) == len(hits)
        hits += [(0, 0, -1, RD), (0, 0, -2, WR)]
        return build(100 + 64 * a_mod + n_mod, 2000, hits, wt=WT, rt=RT + RTW, a_mod=a_mod, n_mod=n_mod)
    if name == "big":
        # 300K later txns x 10 accesses behind a 4,096-txn prefix: past 2.1M
        # accesses k_kill's grid is at its 256-block cap, so waves run two steps
        # and a ragged last one; 5 % of the later accesses touch a marked row
        return build(13, 300_000, [(0, 0, -1, WR), (0, 0, -2, RD)], wt=WT, rt=RT, a_mod=33, n_mod=1, k=4096,
                     mark_frac=0.05)
    raise KeyError(name)


@functools.lru_cache(maxsize=1)
def _dense_table():
    return O.YcsbTable(ROWS)


class _HashedIndex:
    """the oracle's chained index over key 7 * row + 3 -> row (as O.MultiIndex, from arrays)"""

    def __init__(self):
        self.keys = np.arange(ROWS, dtype=np.uint64) * np.uint64(7) + np.uint64(3)
        rows = np.arange(ROWS, dtype=np.uint64)
        L = O.lib()
        self.ix = L.or_index_create(ROWS, 1, 0, ROWS)
        assert L.or_index_insert_many(self.ix, O._p(self.keys, ctypes.c_uint64), O._p(rows, ctypes.c_uint64), ROWS) == 0

    def __del__(self):
        try:
            O.lib().or_index_free(self.ix)
        except Exception:
            pass


@functools.lru_cache(maxsize=1)
def _hashed_index():
    return _HashedIndex()


# (about 17 MB a reference: the cache holds a case's dense and hashed ones)
@functools.lru_cache(maxsize=2)
def _ref(name, cc, hashed):
    case = case_of(name)
    e = case.epoch(hashed)
    f0 = _dense_table().f0.copy()
    ix = _hashed_index().ix if hashed else _dense_table().ix
    c, _, st = O.epoch_run(OCC_ID[cc], ix, f0, e.n_txn, e.txn_begin, e.keys, e.types)
    commit, _, _ = case.facts(cc)
    assert np.array_equal(c, commit), f"{name} {cc}: the oracle is off the formula at {np.flatnonzero(c != commit)[:8]}"
    return c.copy(), (st.committed, st.aborted, st.write_cnt, st.read_digest), f0


@pytest.fixture(scope="module")
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield
    _ref.cache_clear()
    case_of.cache_clear()


def _engine(cc, case, variant):
    eng = CCEngine(CC[cc], case.n_txn, case.n_acc)
    if variant == "hashed":
        eng.create_table(0, ROWS, ROWS, dvcc.HASH_MOD)
        eng.load_table(0, _hashed_index().keys, _dense_table().f0)
    else:
        eng.load_ycsb_partition(ROWS)
    eng.set_prefix(case.k)
    return eng


def _device_epoch(case, variant):
    e = case.epoch(variant == "hashed")
    if variant == "acc_txn":  # no boundaries: k_kill<0> over the probe's acc_row
        return DeviceEpoch.from_tensors(torch.from_numpy(e.keys.view(np.int64)).cuda(), torch.from_numpy(e.types).cuda(),
                                        torch.from_numpy(e.acc_txn().view(np.int32)).cuda(), e.n_txn,
                                        max_txn_acc=e.max_txn_acc())
    dep = DeviceEpoch(e, txn_begin=True, recs32=variant == "recs")
    assert (dep.recs32 is not None) == (variant == "recs")
    return dep


def _check(name, cc, variant, eng=None):
    case = case_of(name)
    c_ref, counts, f0 = _ref(name, cc, variant == "hashed")
    _, surv, kept = case.facts(cc)
    own = eng is None
    eng = eng or _engine(cc, case, variant)
    try:
        d = torch.zeros(case.n_txn, dtype=torch.uint8, device="cuda")
        st = eng.run_epoch_device(_device_epoch(case, variant), d)
        c = d.cpu().numpy()
        print(f"{name} {cc} {variant}: a_acc {case.a_acc} n_acc {case.n_acc} committed {st.committed} "
              f"survivors {st.surv_txn} / {surv} kept {st.surv_acc} / {kept}, {int((c != c_ref).sum())} txns off")
        assert st.prefix_txn == case.k, st.prefix_txn
        assert np.array_equal(c, c_ref), f"{int((c != c_ref).sum())} txns off the oracle, first {np.flatnonzero(c != c_ref)[:8]}"
        assert (st.committed, st.aborted, st.write_cnt, st.read_digest) == counts
        assert (st.surv_txn, st.surv_acc) == (surv, kept)
        if own:
            assert np.array_equal(eng.read_table(0, ROWS), f0), "table state mismatch"
    finally:
        if own:
            eng.close()


SMALL = ["boundary_wr", "boundary_rd", "collide"] + [f"pos_{a}_{n}" for a in (0, 1, 63) for n in (0, 1, 63)]


def test_cases_hold_on_the_oracle():
    """(no engine) every small case's commit bytes on the oracle are the
    formula's, and the cases contain what their names say"""
    for cc in CC:
        for name in SMALL:
            for hashed in (False, True) if name == "collide" else (False,):
                _ref(name, cc, hashed)
    for name in ("boundary_wr", "boundary_rd"):
        case, edge = case_of(name), [HOT - 1, HOT, HOT + 1]
        assert (case.m_wr if name == "boundary_wr" else case.m_rd)[edge].all()
        lr, lt = case.rows[case.a_acc:].astype(np.int64), case.types[case.a_acc:]
        for r in edge:
            assert ((lr == r) & (lt == RD)).sum() == 2 and ((lr == r) & (lt == WR)).sum() == 1
        dead = {cc: int((case.facts(cc)[0] == 0).sum()) for cc in CC}
        # wr: all nine txns die; rd: the three writers die under the locking algorithms, nobody under OCC
        assert dead == ({"NO_WAIT": 9, "WAIT_DIE": 9, "OCC": 9} if name == "boundary_wr"
                        else {"NO_WAIT": 3, "WAIT_DIE": 3, "OCC": 0}), dead
        _, surv, kept = case.facts("NO_WAIT")
        if name == "boundary_rd":  # the six readers survive without those reads
            whole = int(np.diff(case.tb.astype(np.int64))[case.k:][case.facts("NO_WAIT")[0][case.k:] == 1].sum())
            assert whole - kept == 6
    case = case_of("collide")
    (a0, b0), (a1, b1) = colliders(2)
    assert case.m_wr[[a0, a1]].all() and not (case.m_wr | case.m_rd)[[b0, b1, a0 ^ 1, a1 ^ 1]].any()
    assert int((case.facts("OCC")[0] == 0).sum()) == 4  # the four txns on A0 and A1, nobody on their colliders
    for a in (0, 1, 63):
        for n in (0, 1, 63):
            case = case_of(f"pos_{a}_{n}")
            assert (case.a_acc % 64, case.n_acc % 64) == (a, n)
            r = case.rows.astype(np.int64)
            kill = np.flatnonzero(case.m_wr[r] | (case.m_rd[r] & (case.types == WR)))
            kill = kill[kill >= case.a_acc]
            assert kill[0] == case.a_acc and kill[-1] == case.n_acc - 1
            words = (kill >> 6) - (case.a_acc >> 6)
            assert {(int(w) % KILL_WORDS, int(i) % 64) for w, i in zip(words, kill)} >= {
                (q, lane) for q in range(KILL_WORDS) for lane in (0, 31, 63)}


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cc", list(CC))
@pytest.mark.parametrize("name", ["boundary_wr", "boundary_rd"])
def test_hot_cold_boundary(_gpu, name, cc, variant):
    """Rows kHotRows - 1 (the last word of the LDS bitmap copy), kHotRows and
    kHotRows + 1 (the first rows behind the filter), written -- every later
    reader and writer dies -- or only read by the prefix: the later writers
    die under NO_WAIT / WAIT_DIE and the readers' accesses are skipped; under
    OCC all of them survive."""
    _check(name, cc, variant)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cc", list(CC))
def test_false_positive_and_bitmap_neighbour(_gpu, cc, variant):
    """A filter hit that is no bitmap hit: B shares A's filter bit, A ^ 1 A's
    bitmap word, the prefix wrote A alone.  The txns on A die; those that
    read or write B or A ^ 1 survive and commit."""
    _check("collide", cc, variant)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cc", list(CC))
@pytest.mark.parametrize("a_mod", [0, 1, 63])
def test_positions(_gpu, a_mod, cc, variant):
    """The first later access at 64k + a_mod and, one epoch after the other
    on one engine, the epoch's end at 64k + 0, 1 and 63; killing accesses at
    lanes 0, 31 and 63 of every word of a step, at the first later access and
    at the last access of the epoch.  2,000 later txns: three blocks."""
    names = [f"pos_{a_mod}_{n}" for n in (0, 1, 63)]
    eng = _engine(cc, max((case_of(n) for n in names), key=lambda c: c.n_acc), variant)
    try:
        for n in names:  # (every pos case leaves the prefix's and the survivors' writes: a fresh table each)
            if variant == "hashed":
                eng.load_table(0, _hashed_index().keys, _dense_table().f0)
            else:
                eng.load_ycsb_partition(ROWS)
            _check(n, cc, variant, eng)
            assert np.array_equal(eng.read_table(0, ROWS), _ref(n, cc, variant == "hashed")[2]), "table state mismatch"
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("variant,cc", [(v, "NO_WAIT") for v in VARIANTS] + [("recs", "WAIT_DIE"), ("recs", "OCC")])
def test_grid_cap_ragged_steps(_gpu, variant, cc):
    """3M accesses: the 256-block grid cap, two full steps a wave and a ragged
    third, so the records prefetched behind a step's gathers are the next
    step's; 4,096 prefix txns mark 20K rows, and 5 % of the later accesses
    touch one of them."""
    _check("big", cc, variant)
