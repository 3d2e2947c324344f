"""tests/loop_cases.py on the CPU: the constants parse, each size reaches the
edge it is named for (by arithmetic over the parsed constants), the commit
formula against the oracle for every epoch the GPU tests run at the 65k sizes
(and two epochs at per_loop), and the models over the hot-row pool --
conservation, no txn in flight twice, the seeded epoch's closed form, D = 1
equal to the plain tracked loop -- with the conditions the GPU tests rely on
(nothing lost, the log not overflowed, slot_cap >= fullest) asserted here.
"""
import numpy as np
import pytest

import dvcc
import loop_cases as LC
from test_carry import host_closed_loop, host_closed_loop_lanes
from test_loop_backoff import BackoffModel
from test_loop_backoff_lanes import LanesBackoffModel
from test_loop_track import TrackModel

import _oracle as O

K = LC.constants()
S = LC.sizes(K)
T = K["kCarryTpb"]
CCS = [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC]


def test_constants_parse():
    assert K["kCarryTpb"] == K["kBlock"] and K["kTrackPer"] * 64 == K["kCarryTpb"]
    assert K["kR"] >= 2 and K["kTrackSlots"] >= 2 and K["kBoClasses"] == 5
    assert K["kTrackBins"] > 255  # (a commit with abort count 255 has a bin of its own)
    assert K["track_fresh_cap"] == K["bo_spill_cap"] and K["refill_fresh_cap"] > K["track_fresh_cap"]
    # ten bits a class hold a whole carry block of one class
    assert T <= 1023


def test_each_size_reaches_its_edge():
    kR, B = K["kR"], K["kBlock"]
    # full_1: per = 1 and every scan thread holds one count
    assert (LC.per_of(S["full_1"], K), LC.scan_path(S["full_1"], K)) == (1, "one")
    assert LC.n_blocks(S["full_1"], K) == B and LC.thread_chunks(S["full_1"], K) == (None, None)
    assert LC.track_groups(S["full_1"], K) == 2 * K["kTrackSlots"]  # every copy used twice
    # per_2: thread T/2 holds one count of its two, later threads none; the last block holds one txn
    assert (LC.per_of(S["per_2"], K), LC.scan_path(S["per_2"], K)) == (2, "registers")
    assert LC.thread_chunks(S["per_2"], K) == (B // 2, B // 2 + 1)
    assert S["per_2"] - (LC.n_blocks(S["per_2"], K) - 1) * T == 1
    assert LC.track_groups(S["per_2"], K) == 2 * K["kTrackSlots"] + 1  # copy 0 three times
    # per_kR: the top of the register path, every thread a full chunk
    assert (LC.per_of(S["per_kR"], K), LC.scan_path(S["per_kR"], K)) == (kR, "registers")
    assert LC.thread_chunks(S["per_kR"], K) == (None, None)
    # per_loop: the loop path, a thread with one count, threads with none, a ragged last block
    n = S["per_loop"]
    nb = LC.n_blocks(n, K)
    assert (LC.per_of(n, K), LC.scan_path(n, K)) == (kR + 1, "loop") and nb == kR * T + 2
    short, none = LC.thread_chunks(n, K)
    assert nb - short * (kR + 1) == 1 and none == short + 1 < B
    assert n - (nb - 1) * T == 1
    # the grid caps: second grid-stride passes
    assert LC.grid_passes(n, K["track_fresh_cap"], K) >= 2           # k_track_fresh over n_out
    assert LC.grid_passes(n, K["refill_fresh_cap"], K) == 2          # k_refill_fresh: n single-access fresh txns
    assert LC.grid_passes(S["per_kR"], K["refill_fresh_cap"], K) == 1
    assert LC.grid_passes(S["per_2"], K["track_fresh_cap"], K) == 1
    spill = K["bo_spill_cap"] * B + 1
    assert LC.grid_passes(spill, K["bo_spill_cap"], K) == 2
    for name in S:
        assert LC.track_groups(S[name], K) > K["kTrackSlots"], name


@pytest.mark.parametrize("name", list(S))
def test_scan_chunks_of_the_first_epoch(name):
    """epoch 0 from cursor 0: the block counts k_carry_scan / k_bo_scan meet
    hold a chunk that sums to zero and one that sums to per T, and all five
    block kinds"""
    n, p = S[name], LC.pool(name)
    per, nb = LC.per_of(n, K), LC.n_blocks(n, K)
    dead = LC.formula(p.hw[:n]) == 0
    bt = np.add.reduceat(dead.astype(np.int64), np.arange(0, n, T))
    assert len(bt) == nb
    pad = np.concatenate([bt, np.zeros(per * K["kBlock"] - nb, np.int64)]).reshape(K["kBlock"], per).sum(1)
    held = np.clip(nb - np.arange(K["kBlock"]) * per, 0, per)
    assert ((pad == 0) & (held == per)).any(), "no whole chunk sums to zero"
    assert (pad == per * T).any(), "no chunk of per * T"
    assert {0, 1, T - 1, T}.issubset(set(bt.tolist())) and ((bt > 1) & (bt < T - 1)).any()
    if p.lens.min() == 0:  # empty txns, none of them an H-writer
        assert (p.lens[:n] == 0).sum() > n // 16 and (p.lens[p.hw] >= 1).all()


def test_seed_patterns_fill_the_packed_fields():
    """a carry block of T aborts of one class in each field of c012 and c34
    that a whole block can fill, a lane of four classes, counts 253 .. 255"""
    for D, head in ((16, 255), (16, 0), (4, 255), (4, 0)):
        lgD = D.bit_length() - 1
        ab = LC.seed_aborts(2000, T, head)
        cls = np.minimum(ab, lgD)
        for blk, want in ((1, 0), (2, 2), (3, min(3, lgD)), (4, min(4, lgD))):
            assert (cls[blk * T:(blk + 1) * T] == want).all()  # (all T abort: the commit is in block 0)
        lane = cls[5 * T:5 * T + K["kTrackPer"]]
        assert len(set(lane.tolist())) == min(K["kTrackPer"], lgD + 1)
        assert ab[6 * T:6 * T + 4].tolist() == [253, 254, 255, 255] and ab[0] == head
        assert set(cls[:T].tolist()) == set(range(lgD + 1))


@pytest.mark.parametrize("name", ["full_1", "per_2"])
@pytest.mark.parametrize("cc", CCS)
def test_formula_against_the_oracle_tracked(name, cc):
    """the plain / tracked loops of the GPU file: 3 epochs (full_1 with the
    cursor wrapping), every epoch decided by the oracle and the formula"""
    n, p = S[name], LC.pool(name)
    cur0 = p.P - 1000 if name == "full_1" else 0
    m = TrackModel(p.P, cur0, n, n_bins=8)
    ref, left, f0 = LC.run_model(cc, p, m, 3)
    assert all(c.sum() == (~p.hw[h_src]).sum() + 1 for (c, _, _), h_src in zip(ref, [m.seen[k][0] for k in range(3)]))
    assert m.pos == m.totals[0] and m.totals[0] + m.totals[1] == 3 * n
    if name == "full_1":
        assert m.seen[0][0][999] == p.P - 1 and m.seen[0][0][1000] == 0  # the pool wraps inside the first take
    # the same loop by tests/test_carry.py's host loop
    tab = O.YcsbTable(p.rows)
    g0 = tab.f0.copy()
    plain, pnxt, pcur = host_closed_loop(cc, tab, g0, p.epoch, cur0, n, 3)
    for (c, _, h), (pc, _, ph) in zip(ref, plain):
        assert np.array_equal(c, pc) and np.array_equal(h.keys, ph.keys) and np.array_equal(h.txn_begin, ph.txn_begin)
    assert pcur == m.cur and np.array_equal(g0, f0) and np.array_equal(pnxt.keys, left[3].keys)


def test_formula_against_the_oracle_per_loop():
    n, p = S["per_loop"], LC.pool("per_loop")
    m = TrackModel(p.P, 0, n, n_bins=8)
    ref, left, f0 = LC.run_model(dvcc.NO_WAIT, p, m, 2)
    assert ref[0][2].n_acc == n > K["refill_fresh_cap"] * K["kBlock"]  # single-access txns, all fresh
    assert m.totals[1] > 0 and m.cur < p.P


def _conserved(m, extra=()):
    """every txn drawn or seeded is in an epoch, in exactly one slot, or in the log"""
    held = [m.ep[0] | m.ep[1] << 32] + [s[0] | s[1] << 32 for s in m.slots] + [m.log_words()]
    drawn = np.concatenate(list(m.drawn) + [np.asarray(e, np.int64) for e in extra])
    assert len(np.unique(drawn)) == len(drawn)
    assert np.array_equal(np.sort(np.concatenate(held)), np.sort(drawn))
    assert len(np.unique(drawn & 0xFFFFFFFF)) == len(drawn), "a pool txn drawn twice"


@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.OCC])
@pytest.mark.parametrize("D", [1, 2, 4, 16])
def test_backoff_model_over_the_pool(cc, D):
    n, p = S["per_2"], LC.pool("per_2")
    m = BackoffModel(p.P, 0, n, D, n_bins=8)
    m.build()
    ref, left, f0 = LC.run_model(cc, p, m, 4)
    _conserved(m)
    assert m.lost == 0 and m.fullest <= m.slot_cap and m.pos == m.totals[0] <= n * 4
    assert m.totals[0] + m.totals[1] == 4 * n
    if D == 1:  # the plain tracked loop
        t = TrackModel(p.P, 0, n, n_bins=8)
        tref, tleft, g0 = LC.run_model(cc, p, t, 4)
        for (c, _, h), (tc, _, th) in zip(ref, tref):
            assert np.array_equal(c, tc) and np.array_equal(h.keys, th.keys)
        assert np.array_equal(m.log_words(), t.log_words()) and m.totals == t.totals and m.cur == t.cur
        assert np.array_equal(m.hist, t.hist) and np.array_equal(m.words(4), t.words(4))


def test_lanes_models_over_the_pool():
    n, p, lanes = S["per_2"], LC.pool("per_2"), 2
    m = LanesBackoffModel(p.P, 0, n, 4, lanes, n_bins=8)
    m.start()
    ref, left, f0 = LC.run_model(dvcc.NO_WAIT, p, m, 4, lanes=lanes)
    _conserved(m)
    assert m.lost == 0 and m.fullest <= m.slot_cap and sorted(left) == [4, 5]
    # D = 1 over two lanes: host_closed_loop_lanes and the lanes tracker
    m1 = LanesBackoffModel(p.P, 0, n, 1, lanes, n_bins=8)
    m1.start()
    r1, l1, g1 = LC.run_model(dvcc.NO_WAIT, p, m1, 4, lanes=lanes)
    t = TrackModel(p.P, 0, n, lanes=lanes, n_bins=8)
    rt, lt, gt = LC.run_model(dvcc.NO_WAIT, p, t, 4, lanes=lanes)
    tab = O.YcsbTable(p.rows)
    g0 = tab.f0.copy()
    plain, pnxt, pcur = host_closed_loop_lanes(dvcc.NO_WAIT, tab, g0, p.epoch, 0, n, 4, lanes)
    for (c, _, h), (tc, _, th), (pc, _, ph) in zip(r1, rt, plain):
        assert np.array_equal(c, tc) and np.array_equal(c, pc)
        assert np.array_equal(h.keys, th.keys) and np.array_equal(h.keys, ph.keys)
    assert m1.cur == t.cur == pcur and np.array_equal(m1.log_words(), t.log_words())
    assert np.array_equal(g0, g1) and np.array_equal(l1[5].keys, pnxt[5].keys)


SEEDED = [(16, 255, 2000), (16, 0, 2000), (4, 255, 2000), (4, 0, 2000)]


@pytest.mark.parametrize("D,head,c", SEEDED)
def test_seeded_epoch_closed_form(D, head, c):
    n, p = S["per_2"], LC.pool("per_2")
    ent = LC.seed_entries(p, c, head)
    m = LC.seed_model(BackoffModel(p.P, 0, n, D, n_bins=K["kTrackBins"], first_epoch=LC.E0), ent)
    src, born, ab = m.build()
    assert m.released == c and np.array_equal(src[:c], ent[0]) and np.array_equal(ab[:c], ent[2])
    assert np.array_equal(src[c:], np.arange(n - c)) and (born[c:] == LC.E0).all() and (born[:c] < LC.E0).all()
    assert ent[0].min() > 3 * n  # the seeds: pool txns the loop never draws
    want_c, parked = LC.seeded_closed_form(p, ent, src[c:], D)
    after = {}
    for s, (psrc, pborn, pab) in parked.items():
        after[s] = len(m.slots[s][0])
        assert after[s] == 0
    ref, left, f0 = LC.run_model(dvcc.NO_WAIT, p, m, 1)
    assert np.array_equal(ref[0][0], want_c) and want_c[0] == 1 and want_c[1:c].sum() == 0
    # the commit of the entry at position 0 is binned by its count, saturated at 255
    assert m.hist[min(head, K["kTrackBins"] - 1)] >= 1 and m.totals[3] == head
    lgD = D.bit_length() - 1
    for q in range(lgD + 1):
        s = (LC.E0 + (1 << q)) % D
        psrc, pborn, pab = parked[s]
        if s == (LC.E0 + 1) % D:  # released at once into epoch E0 + 1, ahead of its fresh txns
            got = tuple(a[:m.released] for a in m.ep)
        else:
            got = m.slots[s]
        assert np.array_equal(got[0], psrc) and np.array_equal(got[1], pborn) and np.array_equal(got[2], pab), q
        assert (len(psrc) >= T or q == 1) and pab.max() <= 255  # (class 1 has no whole block of its own)
    assert max(int(x[2].max()) for x in parked.values()) == 255  # 254 + 1 and 255 + 1 both stored as 255
    _conserved(m, extra=[ent[0] | ent[1] << 32])
    ref2, left, f0 = LC.run_model(dvcc.NO_WAIT, p, m, 1)
    _conserved(m, extra=[ent[0] | ent[1] << 32])
    assert m.lost == 0 and m.fullest <= m.slot_cap


def test_seeded_spill_passes_the_grid_cap():
    n = S["per_2"]
    c = n + K["bo_spill_cap"] * K["kBlock"] + 1
    p = LC.pool("per_2", P=6 * n + 1_000_000)
    ent = LC.seed_entries(p, c, 255)
    assert ent[0].min() > 3 * n
    m = LC.seed_model(BackoffModel(p.P, 0, n, 2, n_bins=8, first_epoch=LC.E0, slot_cap=2 * c), ent)
    src, born, ab = m.build()
    assert m.released == n and m.spilled == c - n and np.array_equal(src, ent[0][:n])
    assert LC.grid_passes(m.spilled, K["bo_spill_cap"], K) == 2
    assert np.array_equal(m.slots[(LC.E0 + 1) % 2][0], ent[0][n:])
    ref, left, f0 = LC.run_model(dvcc.NO_WAIT, p, m, 2)
    _conserved(m, extra=[ent[0] | ent[1] << 32])
    assert m.lost == 0 and c <= m.fullest < 2 * c
