"""The row-queue sort on its own (dv_sort_rows_device: the epoch's sort_rows
call on given keys) against numpy's stable argsort, bit for bit, over the key
sets, sizes and placed buckets of tests/sort_cases.py -- for every key width
from 1 to 32 bits, with and without DV_FLAG_LSD_SORT, with the count on the
host and on the device.  Every call also asserts the launches the hand-written
path table expects, and three properties that hold whatever the path: the
output is a permutation of the input, every row's keys are contiguous, and a
row's keys keep their input order.  test_sort_cases_cpu.py holds the
reference, the table and the generators to plain Python.
"""
import numpy as np
import pytest
import torch

import sort_cases as S
import dvcc
from dvcc import CCEngine
from test_golden import TO_DV, _load
from test_gpu_parity import _gpu_epoch

pytestmark = pytest.mark.gpu

ERR_ARG = dvcc._lib.DV_ERR_ARG
SENTINEL = 0x5A5A5A5A5A5A5A5A  # what d_out holds before a call (no key of a case: their payloads are below 2^22)
TILE = S.K["kTile"]
FLAGS = [False, True]
COUNT_BOUND = 3 * TILE  # a device count's bound lies this far above it


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    yield


def _engine(max_acc, lsd):
    return CCEngine(dvcc.NO_WAIT, 16, max_acc, lsd_sort=lsd)


def _dev(keys):
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).cuda()


def _sort(eng, keys, key_bits, lsd, count=None, what=""):
    """one call: keys[0, n) with the count on the host (count None) or on the
    device (n its bound); checks launches, the order, the properties and that
    nothing past the real count is written as a result"""
    n = len(keys)
    d_n = torch.tensor([count], dtype=torch.int32, device="cuda") if count is not None else None
    d_out = torch.full((max(n, 1),), SENTINEL, dtype=torch.int64, device="cuda")
    _, launches = eng.sort_rows(_dev(keys), key_bits, d_n, d_out[:n])
    path, want_launches, _ = S.expected_path(key_bits, n, count is not None, lsd)
    assert launches == (want_launches if n else 0), (what, launches, path)
    m = n if count is None else min(n, count)
    out = d_out.cpu().numpy().view(np.uint64)
    assert (out[m:] == np.uint64(SENTINEL)).all(), f"{what}: written past the real count {m}"
    want = S.expected_order(keys[:m], key_bits, path)
    bad = np.flatnonzero(out[:m] != want)
    assert not len(bad), f"{what}: {len(bad)} of {m} keys out of place, first at {bad[0]} ({path})"
    S.check_row_queues(keys[:m], out[:m])
    return path


# ---------------------------------------------------------------- every width, every key set, every size
@pytest.mark.parametrize("lsd", FLAGS, ids=["default", "lsd"])
@pytest.mark.parametrize("key_bits", S.ALL_BITS)
def test_key_sets(key_bits, lsd):
    path, _, width = S.expected_path(key_bits, 1, False, lsd)
    eng = _engine(max(S.SIZES), lsd)
    try:
        for name in S.KEY_SETS:
            for n in S.SIZES:
                keys = S.key_set(name, key_bits, n, path, width)
                assert _sort(eng, keys, key_bits, lsd, what=f"{name} n={n}") == path
    finally:
        eng.close()


@pytest.mark.parametrize("lsd", FLAGS, ids=["default", "lsd"])
@pytest.mark.parametrize("key_bits", S.ALL_BITS)
def test_device_counts(key_bits, lsd):
    """the count on the device: at its bound, far below it, zero, and above it
    (then the bound's keys are sorted); past the real count lies a key that
    would show if it were sorted in"""
    path, _, width = S.expected_path(key_bits, 1, True, lsd)
    eng = _engine(max(S.SIZES) + COUNT_BOUND, lsd)
    try:
        for n in S.SIZES:
            for bound in (n, n + COUNT_BOUND):
                base = S.key_set("uniform", key_bits, bound, seed=1)
                for count in sorted({0, 1, n - 1, n, TILE, TILE + 1, bound + 5}):
                    keys = base.copy()
                    keys[min(count, bound):] = np.uint64(S.filler(key_bits))
                    assert _sort(eng, keys, key_bits, lsd, count, f"n={n} bound={bound} count={count}") == path
        # the other key sets at one size with a partial last tile and a far bound
        for name in S.KEY_SETS[1:]:
            n = 4097
            keys = np.concatenate([S.key_set(name, key_bits, n, path, width),
                                   np.full(COUNT_BOUND, S.filler(key_bits), dtype=np.uint64)])
            _sort(eng, keys, key_bits, lsd, n, f"{name} count={n}")
    finally:
        eng.close()


# ---------------------------------------------------------------- placed buckets
@pytest.mark.parametrize("m", S.PLACED_M)
@pytest.mark.parametrize("key_bits,lo", S.PLACED_WIDTHS)
def test_placed_bucket(key_bits, lo, m):
    """exactly m keys in one bucket, every other bucket empty: one, two and
    three passes over the bucket's other hash bits, in LDS (m <= kBucketCap)
    and through global memory, whose even pass counts end in the scratch
    region"""
    assert S.K["kBucketCap"] in S.PLACED_M and S.K["kBucketCap"] + 1 in S.PLACED_M
    assert S.K["kBucketThreads"] in S.PLACED_M and S.K["kBucketThreads"] * S.K["kBucketGroup"] in S.PLACED_M
    eng = _engine(m + COUNT_BOUND, False)
    try:
        for pat in S.PLACED_PATTERNS:
            keys = S.placed_bucket(key_bits, lo, [(5, m, pat)])
            assert _sort(eng, keys, key_bits, False, what=f"{pat} m={m}") == "bucket"
            padded = np.concatenate([keys, np.full(COUNT_BOUND, S.filler(key_bits), dtype=np.uint64)])
            assert _sort(eng, padded, key_bits, False, m, f"{pat} m={m} on the device") == "bucket"
    finally:
        eng.close()


@pytest.mark.parametrize("key_bits,lo", S.PLACED_WIDTHS)
def test_buckets_beside_an_oversized_one(key_bits, lo):
    """digit_pre: a smaller bucket before and after one that is sorted through
    global memory, and the first and the last bucket"""
    last = (1 << lo) - 1
    cap = S.K["kBucketCap"]
    cases = {
        "small after big": [(3, cap + 1, "pairs"), (4, 100, "descending")],
        "small before big": [(9, 100, "descending"), (8, 2 * cap + 1, "descending")],
        "interleaved": [(last, 700, "pairs"), (0, cap + 5, "equal"), (last - 1, 513, "descending"),
                        (0, 64, "descending"), (1, 1, "equal")],
        "first and last": [(last, 8193, "descending"), (0, 8191, "descending")],
        "last is big": [(0, 2, "equal"), (last, cap + 1, "descending")],
    }
    eng = _engine(max(sum(m for _, m, _ in c) for c in cases.values()), False)
    try:
        for what, buckets in cases.items():
            keys = S.placed_bucket(key_bits, lo, buckets)
            assert _sort(eng, keys, key_bits, False, what=what) == "bucket"
            # the same keys dealt round-robin over the buckets
            rng = np.random.default_rng(len(keys))
            mixed = S.with_payload(S.rows_of(keys)[rng.permutation(len(keys))])
            assert _sort(eng, mixed, key_bits, False, len(mixed), what + ", shuffled, on the device") == "bucket"
    finally:
        eng.close()


# ---------------------------------------------------------------- the kBucketMaxN switch
def test_bucket_max_n_switch():
    key_bits, n = 20, S.BUCKET_MAX_N
    assert S.expected_path(key_bits, n) == ("bucket", 2, 8)
    assert S.expected_path(key_bits, n + 1) == ("lsd", 2, 10)
    assert S.expected_path(key_bits, n + 1, on_dev=True) == ("bucket", 2, 8)
    keys = S.key_set("uniform", key_bits, n + 1, seed=2)
    eng = _engine(n + 1, False)
    try:
        assert _sort(eng, S.with_payload(S.rows_of(keys[:n])), key_bits, False, what="n = kBucketMaxN") == "bucket"
        assert _sort(eng, keys, key_bits, False, what="n = kBucketMaxN + 1") == "lsd"
        assert _sort(eng, keys, key_bits, False, n + 1, "n = kBucketMaxN + 1 on the device") == "bucket"
    finally:
        eng.close()


# ---------------------------------------------------------------- refusals, and no state left behind
@pytest.mark.parametrize("lsd", FLAGS, ids=["default", "lsd"])
def test_refusals(lsd):
    L = dvcc._lib.lib()
    import ctypes
    n, key_bits = 1000, 16
    eng = _engine(n, lsd)
    try:
        keys = S.key_set("uniform", key_bits, n, seed=3)
        d_in, d_out = _dev(keys), torch.full((n + 1,), SENTINEL, dtype=torch.int64, device="cuda")
        launches = ctypes.c_uint32(77)
        pin, pout, pl = ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), ctypes.byref(launches)

        def call(ctx, a, nn, kb, o, la):
            return L.dv_sort_rows_device(ctx, a, nn, None, kb, o, la)

        refused = [("null context", call(None, pin, n, key_bits, pout, pl)),
                   ("null keys", call(eng._ctx, None, n, key_bits, pout, pl)),
                   ("null out", call(eng._ctx, pin, n, key_bits, None, pl)),
                   ("null launches", call(eng._ctx, pin, n, key_bits, pout, None)),
                   ("n > max_acc", call(eng._ctx, pin, n + 1, key_bits, pout, pl)),
                   ("key_bits 0", call(eng._ctx, pin, n, 0, pout, pl)),
                   ("key_bits 33", call(eng._ctx, pin, n, 33, pout, pl)),
                   ("key_bits -1", call(eng._ctx, pin, n, -1, pout, pl))]
        for what, rc in refused:
            assert rc == ERR_ARG, (what, rc)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy().view(np.uint64) == np.uint64(SENTINEL)).all(), "a refused call wrote its output"
        with pytest.raises(dvcc.DvccError) as ex:
            eng.sort_rows(torch.zeros(n + 1, dtype=torch.int64, device="cuda"), key_bits)
        assert ex.value.code == ERR_ARG
        # n == 0: DV_OK, nothing launched, nothing written
        assert call(eng._ctx, pin, 0, key_bits, pout, pl) == dvcc._lib.DV_OK and launches.value == 0
        assert (d_out.cpu().numpy().view(np.uint64) == np.uint64(SENTINEL)).all()
        # the context sorts correctly after them
        _sort(eng, keys, key_bits, lsd, what="after the refusals")
        _sort(eng, keys, key_bits, lsd, n - 1, "after the refusals, on the device")
    finally:
        eng.close()


@pytest.mark.parametrize("lsd", FLAGS, ids=["default", "lsd"])
@pytest.mark.parametrize("name", ["nowait_z09", "calvin_z06"])
def test_an_epoch_after_a_sort_is_bit_exact(name, lsd):
    """the entry point leaves no state behind: a golden epoch on the same
    context, after sorts of other keys at another width and count"""
    g = _load(name)
    cc = TO_DV[int(g["cc"])]
    rows = int(g["rows"])
    e = dvcc.Epoch(g["keys"], g["types"], g["txn_begin"])
    eng = CCEngine(cc, e.n_txn, max(e.n_acc, 20000), lsd_sort=lsd)
    try:
        eng.load_ycsb_partition(rows)
        _sort(eng, S.key_set("uniform", 28, 20000, seed=4), 28, lsd, what="before the epoch")
        _sort(eng, S.key_set("bit0_runs", 12, 5000), 12, lsd, 4097, "before the epoch, on the device")
        commit, grant, st = _gpu_epoch(eng, e, "device")
        assert np.array_equal(commit, g["commit"])
        if cc == dvcc.CALVIN:
            assert np.array_equal(grant, g["grant"])
        committed, aborted, digest, wcnt = (int(x) for x in g["stats"])
        assert (st.committed, st.aborted, st.read_digest, st.write_cnt) == (committed, aborted, digest, wcnt)
        assert np.array_equal(eng.read_table(0, rows), g["f0"])
        _sort(eng, S.key_set("descending", 17, 8193), 17, lsd, what="after the epoch")
    finally:
        eng.close()
