"""tests/sort_cases.py on the CPU: the hand-written path table against the
header's rules, the reference against a plain Python sort, the placed-bucket
generator against the hash formula, and the multiplier's inverse.  Nothing
here calls the engine."""
import numpy as np
import pytest

import sort_cases as S

CPU_BITS = S.ALL_BITS


def test_constants_are_the_headers():
    k = S.K
    assert k["kRowHashMul"] == 0x9E3779B1 and k["kRowHashMul"] % 2 == 1
    assert k["kBucketMaxN"] == S.BUCKET_MAX_N
    assert k["kTile"] == 4096 and k["kBucketCap"] == 16384
    assert k["kBucketThreads"] * k["kBucketGroup"] == 8192


@pytest.mark.parametrize("key_bits", S.ALL_BITS)
def test_path_table_is_the_headers(key_bits):
    for lsd in (False, True):
        for on_dev in (False, True):
            for n in (1, 4096, S.BUCKET_MAX_N, S.BUCKET_MAX_N + 1, 1 << 31):
                assert S.expected_path(key_bits, n, on_dev, lsd) == S.header_path(key_bits, n, on_dev, lsd), \
                    (key_bits, n, on_dev, lsd)
    path, launches, w = S.expected_path(key_bits, 1, lsd=True)
    # the passes cover the key and no pass is empty
    assert path == "lsd" and w * (launches - 1) < key_bits <= w * launches


def test_path_table_rows():
    """every row of the table is some call's path, and the switch at kBucketMaxN"""
    assert S.expected_path(8, 100) == ("lsd", 1, 8)
    assert S.expected_path(9, 100) == ("bucket", 2, 8)
    assert S.expected_path(9, 100, lsd=True) == ("lsd", 1, 9)
    assert S.expected_path(27, 100) == ("bucket", 2, 9)
    assert S.expected_path(28, 100) == ("bucket", 2, 10)
    assert S.expected_path(28, 100, lsd=True) == ("lsd", 3, 10)
    assert S.expected_path(29, 100) == ("lsd", 3, 10)
    assert S.expected_path(32, 100) == ("lsd", 4, 8)
    assert S.expected_path(20, S.BUCKET_MAX_N) == ("bucket", 2, 8)
    assert S.expected_path(20, S.BUCKET_MAX_N + 1) == ("lsd", 2, 10)
    assert S.expected_path(20, S.BUCKET_MAX_N + 1, on_dev=True) == ("bucket", 2, 8)


@pytest.mark.parametrize("key_bits", S.ALL_BITS)
def test_multiplier_inverse(key_bits):
    inv, mask = S.mul_inverse(key_bits), (1 << key_bits) - 1
    assert (S.MUL * inv) & mask == 1
    probe = sorted({0, 1, 2 & mask, mask, mask - 1, mask >> 1, (mask >> 1) + 1, 0x12345678 & mask})
    for h in probe:
        assert S.row_hash(S.unhash(h, key_bits), key_bits) == h
    hs = np.array(probe, dtype=np.uint64)
    assert (S.row_hash(S.unhash(hs, key_bits), key_bits) == hs).all()
    assert [int(x) for x in S.unhash(hs, key_bits)] == [S.unhash(h, key_bits) for h in probe]


def _python_sorted(keys, prim):
    order = sorted(enumerate(int(p) for p in prim), key=lambda t: (t[1], t[0]))
    return [int(keys[i]) for i, _ in order]


@pytest.mark.parametrize("key_bits", CPU_BITS)
def test_stable_by_is_a_plain_stable_sort(key_bits):
    for path in ("lsd", "bucket"):
        if path == "bucket" and not 8 < key_bits <= 28:
            continue
        width = S.expected_path(key_bits, 1, lsd=path == "lsd")[2]
        for name in S.KEY_SETS:
            for n in (s for s in S.SIZES if s <= 4097):
                keys = S.key_set(name, key_bits, n, path, width)
                assert len(keys) == n and (S.rows_of(keys) < 1 << key_bits).all()
                assert ((keys & np.uint64(0xFFFFFFFF)) == np.arange(n - 1, -1, -1, dtype=np.uint64)).all()
                prim = S.primary(keys, key_bits, path)
                if path == "bucket":
                    assert [int(p) for p in prim[:50]] == [(int(k) >> 32) * S.MUL % (1 << key_bits) for k in keys[:50]]
                want = S.expected_order(keys, key_bits, path)
                assert [int(x) for x in want] == _python_sorted(keys, prim), (name, n, path)
                S.check_row_queues(keys, want)
                # the payloads tell the stable sort from a sort of the whole word
                if len(np.unique(S.rows_of(keys))) < n and path == "lsd":
                    assert (np.sort(keys) != want).any(), (name, n)


def test_key_sets_are_what_they_say():
    for key_bits in CPU_BITS:
        top = 1 << key_bits
        for name, rows in (("row_0", {0}), ("row_max", {top - 1}), ("bit0_alternating", {top - 1, (top - 1) ^ 1}),
                           ("top_runs", {top - 1, (top - 1) ^ (top >> 1)})):
            got = {int(r) for r in S.rows_of(S.key_set(name, key_bits, 200))}
            assert got == rows, (name, key_bits)
        r = [int(x) for x in S.rows_of(S.key_set("bit0_runs", key_bits, 200))]
        assert r[:65] == [top - 1] * 65 and r[65:130] == [(top - 1) ^ 1] * 65 and r[130] == top - 1
        r = [int(x) for x in S.rows_of(S.key_set("descending", key_bits, 200))]
        if top >= 200:
            assert all(a > b for a, b in zip(r, r[1:])) and r[0] >= top // 2 - 1 and r[-1] == 0
        # one row per digit value of each pass
        _, passes, w = S.expected_path(key_bits, 1, lsd=True)
        d = [int(x) for x in S.digit_rows(key_bits, "lsd", w)]
        for p in range(passes):
            digits = {(x >> (w * p)) & ((1 << w) - 1) for x in d}
            assert digits == set(range(1 << min(w, key_bits - w * p))), (key_bits, p)
        if 8 < key_bits <= 28:
            lo = S.BUCKET_LO[key_bits]
            hb = key_bits - lo
            h = [S.row_hash(int(x), key_bits) for x in S.digit_rows(key_bits, "bucket", lo)]
            assert {x >> hb for x in h} == set(range(1 << lo))
            inside = [x & ((1 << hb) - 1) for x in h if x >> hb == (1 << lo) - 2]
            for p in range((hb + 7) // 8):
                assert {(x >> 8 * p) & 255 for x in inside} == set(range(1 << min(8, hb - 8 * p))), (key_bits, p)


@pytest.mark.parametrize("key_bits,lo", S.PLACED_WIDTHS)
def test_placed_buckets_land_where_stated(key_bits, lo):
    """by the formula, bucket = top lo bits of row * mul mod 2^key_bits"""
    assert lo == S.BUCKET_LO[key_bits]
    hb, mask = key_bits - lo, (1 << key_bits) - 1
    for b in (0, 5, (1 << lo) - 1):
        for m in S.PLACED_M:
            for pat in S.PLACED_PATTERNS:
                keys = S.placed_bucket(key_bits, lo, [(b, m, pat)])
                assert len(keys) == m
                h = [((int(k) >> 32) * S.MUL) & mask for k in keys[:600]] + \
                    [((int(k) >> 32) * S.MUL) & mask for k in keys[-600:]]
                assert {x >> hb for x in h} == {b}
                hv = S.row_hash(S.rows_of(keys), key_bits)
                assert ((hv >> np.uint64(hb)) == b).all() and (S.rows_of(keys) <= mask).all()
                low = hv & np.uint64((1 << hb) - 1)
                assert (low == S.placed_low(m, hb, pat)).all()
                if pat == "equal":
                    assert len(np.unique(low)) == 1
                elif pat == "few_rows":
                    assert len(np.unique(low)) <= 37 and (m < 600 or len(np.unique(low)) >= 2)
                elif pat == "pairs":
                    assert (low[0::2][:m // 2] == low[1::2]).all() and int(low[0]) == (1 << hb) - 1
                    assert len(np.unique(low)) == min((m + 1) // 2, 1 << hb)
                else:
                    assert int(low[0]) == (1 << hb) - 1
                    assert (low[1:][low[:-1] > 0] == low[:-1][low[:-1] > 0] - np.uint64(1)).all()
                    assert len(np.unique(low)) == min(m, 1 << hb)
    two = S.placed_bucket(key_bits, lo, [(3, 20000, "descending"), (7, 100, "equal")])
    hv = S.row_hash(S.rows_of(two), key_bits) >> np.uint64(hb)
    assert (hv[:20000] == 3).all() and (hv[20000:] == 7).all() and len(two) == 20100
