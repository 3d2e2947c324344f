"""The closed loop's refill chain, tracker and back-off on the GPU at the epoch
sizes of tests/loop_cases.py -- where k_carry_scan / k_bo_scan change their
code shape, k_track_carry / k_bo_park share their partial copies between
workgroups, and k_track_fresh / k_refill_fresh / k_bo_spill take a second
grid-stride pass (tests/test_loop_cases_cpu.py proves each by arithmetic).

Every expected commit byte is the numpy formula's, the oracle is asserted
equal to it, and the device is compared exactly to both; identities, rings,
logs and counters come from the numpy models driven by the formula.  The
tracker's and the back-off's arrays are guarded.
"""
import numpy as np
import pytest

import _oracle as O
import loop_cases as LC
from test_loop_backoff import BackoffModel
from test_loop_backoff_lanes import LanesBackoffModel
from test_loop_track import TrackModel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import CCEngine, DeviceEpoch, LoopBackoff, LoopTrack  # noqa: E402
from test_loop_backoff_gpu import _guarded as _guarded_bo, _guards_stand as _guards_stand_bo  # noqa: E402
from test_loop_track_gpu import _check_next, _check_outcomes, _check_track, _guarded, _guards_stand  # noqa: E402

K = LC.constants()
S = LC.sizes(K)
T = K["kCarryTpb"]
CC_NAME = {dvcc.NO_WAIT: "NO_WAIT", dvcc.WAIT_DIE: "WAIT_DIE", dvcc.OCC: "OCC"}
PREFIX = {"off": None, "on": 0}  # (on: the automatic prefix, the tb-form loop)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield
    _dev.clear()


_dev, _refs = {}, {}


def _dev_pool(p):
    """the pool on the device (once per pool, read-only)"""
    if id(p) not in _dev:
        _dev[id(p)] = (p, DeviceEpoch(p.epoch), torch.from_numpy(p.epoch.txn_begin.astype(np.int32)).cuda())
    return _dev[id(p)][1:]


def _ref(key, make):
    """a reference computed once and left unchanged"""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _engine(cc, p, n, prefix):
    eng = CCEngine(cc, n, n * p.epoch.max_txn_acc())
    eng.set_prefix(prefix)
    eng.load_ycsb_partition(p.rows)
    return eng


def _commit_bufs(n, e):
    return [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(e)]


def _got(commits, sts):
    return [(c.cpu().numpy(), s) for c, s in zip(commits, sts)]


# ---- 1. dv_epoch_carry ---------------------------------------------------------
def _carry_cap(p, n):
    """a cap that cuts inside a carry block in the middle of a scan chunk: 100
    txns into the first all-H-writer block whose number is 1 mod per (or any,
    per = 1)"""
    per = LC.per_of(n, K)
    dead = LC.formula(p.hw[:n]) == 0
    bt = np.add.reduceat(dead.astype(np.int64), np.arange(0, n, T))
    b = next(int(b) for b in np.flatnonzero(bt == T) if per == 1 or b % per == 1)
    return int(bt[:b].sum()) + 100


@pytest.mark.parametrize("name,cc", [("full_1", dvcc.NO_WAIT), ("full_1", dvcc.OCC), ("per_2", dvcc.NO_WAIT),
                                     ("per_2", dvcc.OCC), ("per_kR", dvcc.NO_WAIT), ("per_loop", dvcc.NO_WAIT)],
                         ids=lambda v: CC_NAME.get(v, v))
def test_carry(name, cc):
    """the epoch of pool txns 0 .. n - 1, then eng.carry with cap = all and a
    cap inside a scan chunk: the H-writers but the first, in order, renumbered;
    the carried epoch runs and matches the formula"""
    n, p = S[name], LC.pool(name)
    src = np.arange(n, dtype=np.int64)
    tab = O.YcsbTable(p.rows)
    f0 = tab.f0.copy()
    c0, st0, host = LC.decide(cc, p, tab, f0, src)
    cap_in = _carry_cap(p, n)
    assert 0 < cap_in < int((c0 == 0).sum())
    eng = _engine(cc, p, n, 0)
    try:
        dev = DeviceEpoch(host)
        d_commit = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st = eng.run_epoch_device(dev, d_commit)
        _check_outcomes([(d_commit.cpu().numpy(), st)], [(c0, st0, host)])
        carried = {}
        for cap in (n, cap_in):
            csrc, hc = LC.carried_form(p, src, cap)
            assert hc.n_txn == min(cap, int((c0 == 0).sum())) and p.hw[csrc].all()
            dc = eng.carry(dev, cap)
            assert (dc.n_txn, dc.n_acc) == (hc.n_txn, hc.n_acc), cap
            assert np.array_equal(dc.keys.cpu().numpy().view(np.uint64), hc.keys), cap
            assert np.array_equal(dc.types.cpu().numpy(), hc.types), cap
            assert np.array_equal(dc.acc_txn.cpu().numpy().view(np.uint32), hc.acc_txn()), cap
            carried[cap] = (csrc, dc)
        csrc, dc = carried[n]
        c1, st1, h1 = LC.decide(cc, p, tab, f0, csrc)
        assert int(c1.sum()) == 1 and c1[0] == 1
        d1 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st = eng.run_epoch_device(dc, d1)
        _check_outcomes([(d1.cpu().numpy()[:h1.n_txn], st)], [(c1, st1, h1)])
        assert np.array_equal(eng.read_table(0, p.rows), f0)
    finally:
        eng.close()


# ---- 2 / 3. the plain loop, then the same loop tracked ---------------------------
def _tracked_ref(name, cc, e, cur0, n_bins):
    def make():
        p = LC.pool(name)
        m = TrackModel(p.P, cur0, S[name], n_bins=n_bins)
        ref, left, f0 = LC.run_model(cc, p, m, e)
        return p, m, ref, left[e], f0
    return _ref(("tracked", name, cc, e, cur0, n_bins), make)


def _run_loop(name, cc, prefix, e, cur0, n_bins, tracked):
    n = S[name]
    p, m, ref, nxt, f0 = _tracked_ref(name, cc, e, cur0, n_bins)
    assert m.pos == m.totals[0]  # (log_cap below: the log is not overflowed)
    eng = _engine(cc, p, n, prefix)
    try:
        trk = held = None
        if tracked:
            trk = LoopTrack(n, 2, log_cap=m.pos, epoch_cap=e, n_bins=n_bins)
            held = _guarded(trk)
            trk.attach(eng)
        dpool, pb = _dev_pool(p)
        cursor = torch.full((1,), cur0, dtype=torch.int32, device="cuda")
        commits = _commit_bufs(n, e)
        sts, bufs, cursor = eng.closed_loop(dpool, pb, n, e, cursor=cursor, d_commits=commits, track=trk)
        _check_outcomes(_got(commits, sts), ref)
        assert int(cursor.item()) == m.cur
        if e & 1:
            bufs.swap()
            if tracked:
                trk.swap()
        _check_next(bufs, nxt, n, p.epoch)
        assert np.array_equal(eng.read_table(0, p.rows), f0)
        if tracked:
            _check_track(trk, m)
            assert trk.overflowed() == 0
            assert np.array_equal(trk.ids[0][:n].cpu().numpy(), m.words(e))
            assert np.array_equal(trk.ids[1][:n].cpu().numpy(), m.words(e - 1))
            _guards_stand(trk, held)
    finally:
        eng.close()


@pytest.mark.parametrize("prefix", ["off", "on"])
@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC], ids=lambda v: CC_NAME[v])
@pytest.mark.parametrize("name", ["full_1", "per_2"])
def test_plain_then_tracked(name, cc, prefix):
    """3 epochs, the keys form (prefix off) and the tb / recs32 form (on); at
    full_1 the cursor starts 1,000 txns before the pool's end and wraps inside
    the first take; 8 bins with the prefix off, kTrackBins with it on"""
    p = LC.pool(name)
    cur0 = p.P - 1000 if name == "full_1" else 0
    n_bins = 8 if prefix == "off" else K["kTrackBins"]
    _run_loop(name, cc, PREFIX[prefix], 3, cur0, n_bins, tracked=False)
    _run_loop(name, cc, PREFIX[prefix], 3, cur0, n_bins, tracked=True)


@pytest.mark.parametrize("name", ["per_kR", "per_loop"])
def test_tracked_1m(name):
    """NO_WAIT, 2 epochs of single-access txns (three refills): the top of the
    scans' register path and their loop path; at per_loop the second passes of
    k_track_fresh and (first refill: every txn fresh) k_refill_fresh"""
    _run_loop(name, dvcc.NO_WAIT, 0, 2, 0, 8, tracked=True)


# ---- 4 / 5. back-off, one context ------------------------------------------------
def _ring_matches(trk, bo, m, n, bufs_of):
    """every slot's contents and count, the counters, and the identity and
    abort arrays of the buffers bufs_of = [(buffer, epoch)]"""
    torch.cuda.synchronize()
    cnt = bo.slot_count.cpu().numpy().view(np.uint32)
    assert list(cnt) == [len(s[0]) for s in m.slots]
    for s, ((src, born, ab), (msrc, mborn, mab)) in enumerate(zip(bo.parked(), m.slots)):
        assert np.array_equal(src, msrc) and np.array_equal(born, mborn), f"slot {s}"
        assert np.array_equal(ab, mab.astype(np.uint8)), f"slot {s}: aborts"
    assert bo.counters() == m.counters()
    for b, k in bufs_of:
        assert np.array_equal(trk.ids[b][:n].cpu().numpy(), m.words(k)), f"ids of epoch {k}"
        assert np.array_equal(bo.aborts[b][:n].cpu().numpy(), m.aborts_of(k)), f"aborts of epoch {k}"


def _backoff_ref(name, cc, e, D, n_bins, seed=None, P=None):
    """seed: (c, head) -- a ring seeded at epoch E0 (tests/loop_cases.py)"""
    def make():
        p = LC.pool(name, P=P)
        first = LC.E0 if seed else 0
        ent = LC.seed_entries(p, *seed) if seed else None
        cap = 2 * seed[0] if seed and seed[0] > S[name] else None
        m = BackoffModel(p.P, 0, S[name], D, n_bins=n_bins, first_epoch=first, slot_cap=cap)
        if seed:
            LC.seed_model(m, ent)
        m.build()
        ref, left, f0 = LC.run_model(cc, p, m, e)
        assert m.lost == 0
        return p, m, ref, left[first + e], f0, ent
    return _ref(("backoff", name, cc, e, D, n_bins, seed, P), make)


def _run_backoff(name, cc, prefix, e, D, n_bins, seed=None, P=None):
    n = S[name]
    p, m, ref, nxt, f0, ent = _backoff_ref(name, cc, e, D, n_bins, seed, P)
    first = LC.E0 if seed else 0
    slot_cap = max(m.fullest, 1) if seed and seed[0] > n else None  # (the spilling ring: as small as the model allows)
    assert m.lost == 0 and m.pos == m.totals[0]
    eng = _engine(cc, p, n, prefix)
    try:
        trk = LoopTrack(n, 2, log_cap=m.pos, epoch_cap=e, n_bins=n_bins)
        bo = LoopBackoff(trk, D, slot_cap=slot_cap)
        assert bo.slot_cap >= m.fullest
        held = _guarded_bo(trk, bo)
        if seed:  # a ring the caller filled: slot E0 % D
            c, s = len(ent[0]), LC.E0 % D
            bo.park_ids[s * bo.slot_cap:s * bo.slot_cap + c] = torch.from_numpy(ent[0] | ent[1] << 32).cuda()
            bo.park_aborts[s * bo.slot_cap:s * bo.slot_cap + c] = torch.from_numpy(ent[2].astype(np.uint8)).cuda()
            bo.slot_count[s] = c
        trk.attach(eng, first_epoch=first)
        bo.attach(eng)
        dpool, pb = _dev_pool(p)
        commits = _commit_bufs(n, e)
        sts, bufs, cursor = eng.closed_loop(dpool, pb, n, e, d_commits=commits, track=trk)
        _check_outcomes(_got(commits, sts), ref)
        assert int(cursor.item()) == m.cur
        if e & 1:
            bufs.swap()
            trk.swap()
            bo.swap()
        _check_next(bufs, nxt, n, p.epoch)
        assert np.array_equal(eng.read_table(0, p.rows), f0)
        _check_track(trk, m)
        assert trk.overflowed() == 0
        _ring_matches(trk, bo, m, n, [(0, m.k), (1, m.k - 1)])
        _guards_stand_bo(held)
        return trk, bo, m, p, ent, ref
    finally:
        eng.close()


@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.OCC], ids=lambda v: CC_NAME[v])
@pytest.mark.parametrize("D", [2, 4, 16])
def test_backoff_per_2(D, cc):
    """4 epochs from an empty ring; NO_WAIT in the tb form, OCC in the keys form"""
    _run_backoff("per_2", cc, 0 if cc == dvcc.NO_WAIT else None, 4, D, 8)


def test_backoff_per_loop():
    """D = 4, NO_WAIT, 2 epochs (three refills): k_bo_scan's loop path over the
    class rows and over the gather's block counts"""
    _run_backoff("per_loop", dvcc.NO_WAIT, 0, 2, 4, 8)


@pytest.mark.parametrize("D,head,n_bins", [(16, 255, K["kTrackBins"]), (16, 0, 8), (4, 255, 8),
                                          (4, 0, K["kTrackBins"])])
def test_seeded_ring(D, head, n_bins):
    """a ring filled by the caller before epoch 16: whole carry blocks of one
    delay class in each packed field, a lane of four classes, counts 253 ..
    255, the head entry -- the seeded epoch's commit -- with count 255 or 0.
    One refill and one further epoch; the seeded epoch against its closed form"""
    c, e = 2000, 2
    trk, bo, m, p, ent, ref = _run_backoff("per_2", dvcc.NO_WAIT, 0, e, D, n_bins, seed=(c, head))
    n = S["per_2"]
    want_c, parked = LC.seeded_closed_form(p, ent, np.arange(n - c, dtype=np.int64), D)
    assert np.array_equal(ref[0][0], want_c)  # (the device's bytes were held to ref above)
    # the head commits with its count; epoch E0 + 1's commit is the first class-0 abort of epoch E0, count 1
    assert int(m.hist[min(head, n_bins - 1)]) >= 1 and m.totals[3] == max(head, 1)
    slots = bo.parked()
    for q in range(D.bit_length()):
        d = 1 << q
        psrc, pborn, pab = parked[(LC.E0 + d) % D]
        assert len(psrc) > 0
        if d <= e:  # already released: the head of epoch E0 + d, the call's epoch d, in buffer d & 1
            src = trk.ids[d & 1][:len(psrc)].cpu().numpy()
            src, born, ab = src & 0xFFFFFFFF, src >> 32, bo.aborts[d & 1][:len(psrc)].cpu().numpy()
        else:       # still parked, ahead of what the next epoch's park appended
            src, born, ab = (a[:len(psrc)] for a in slots[(LC.E0 + d) % D])
        assert np.array_equal(src, psrc) and np.array_equal(born, pborn) and np.array_equal(ab, pab), q


def test_seeded_ring_spills_past_the_grid_cap():
    """D = 2, n_txn + 262,144 + 1 entries in slot 0: the whole seeded epoch is
    released entries and k_bo_spill moves the rest in two grid-stride passes"""
    n = S["per_2"]
    c = n + K["bo_spill_cap"] * K["kBlock"] + 1
    trk, bo, m, p, ent, ref = _run_backoff("per_2", dvcc.NO_WAIT, 0, 2, 2, 8, seed=(c, 255), P=6 * n + 1_000_000)
    assert m.spilled >= c - n and LC.grid_passes(c - n, K["bo_spill_cap"], K) == 2


# ---- 6. two decision lanes -----------------------------------------------------
def test_two_lanes_tracked_with_backoff():
    """per_2, NO_WAIT, D = 4, 4 epochs over two lanes: one ring and one set of
    partial copies shared by the lanes' refills at more than kTrackSlots
    workgroups"""
    name, cc, lanes, D, e, n_bins = "per_2", dvcc.NO_WAIT, 2, 4, 4, 8
    n = S[name]

    def make():
        p = LC.pool(name)
        m = LanesBackoffModel(p.P, 0, n, D, lanes, n_bins=n_bins)
        m.start()
        ref, left, f0 = LC.run_model(cc, p, m, e, lanes=lanes)
        return p, m, ref, left, f0
    p, m, ref, left, f0 = _ref(("lanes", name, cc, e, D), make)
    assert m.lost == 0 and m.pos == m.totals[0] and e % (2 * lanes) == 0
    eng = _engine(cc, p, n, 0)
    extra = [eng.open_lane() for _ in range(lanes - 1)]
    try:
        trk = LoopTrack(n, 2 * lanes, log_cap=m.pos, epoch_cap=e, n_bins=n_bins)
        bo = LoopBackoff(trk, D)
        assert bo.slot_cap >= m.fullest
        held = _guarded_bo(trk, bo)
        trk.attach(eng)
        bo.attach(eng)
        dpool, pb = _dev_pool(p)
        commits = _commit_bufs(n, e)
        sts, bufs, cursor = eng.closed_loop_lanes(extra, dpool, pb, n, e, d_commits=commits, track=trk)
        _check_outcomes(_got(commits, sts), ref)
        assert int(cursor.item()) == m.cur
        for ln in range(lanes):
            _check_next(bufs[ln], left[e + ln], n, p.epoch)
        assert np.array_equal(eng.read_table(0, p.rows), f0)
        _check_track(trk, m)
        assert trk.overflowed() == 0
        _ring_matches(trk, bo, m, n, [(b, k) for ln in range(lanes)
                                      for b, k in ((2 * ln, m.k + ln), (2 * ln + 1, m.k - lanes + ln))])
        _guards_stand_bo(held)
    finally:
        eng.close()
