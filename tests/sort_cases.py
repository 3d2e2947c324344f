"""Keys, reference and expected path for the row-queue sort on its own (a plain
module, shared by test_sort_cases_cpu.py and test_sort_cases_gpu.py).

A sort key is row << 32 | payload.  The engine sorts stably by row; what it
promises about the order AMONG rows depends on the path:
  LSD     ascending by row                                 primary = keys >> 32
  bucket  ascending by the row's hash h = row * kRowHashMul mod 2^key_bits
          (a stable pass on h's top `lo` bits, then inside each bucket a
          stable sort of h's remaining bits, is a stable sort by all of h)
The reference is numpy's stable argsort of that primary and nothing else.

The payload of key i is n - 1 - i: it DEscends with the input position, so a
comparison sort of the whole 64-bit word (stable or not) reverses every row's
queue and differs from the stable sort wherever a row repeats.

The expected path of a call -- which kernels run and how many timed launches
dv_sort_rows_device reports -- is written out by hand below (LSD_PASSES,
NINE_BIT, TEN_BIT, expected_path) and never computed by the header's own
functions; test_sort_cases_cpu.py holds it to a line-by-line restatement of
them (header_path).
"""
import os
import re

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva-plus_amd", "csrc")


def _src(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _const(text, name):
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)" % name, text).group(1))


def structural_constants():
    """kRowHashMul, kRadixBits, kRadixMaxBits, kBucketHiMax, kBucketMaxN, kTile
    (a radix workgroup's keys), kBucketThreads, kBucketGroup and kBucketCap
    (the keys a workgroup sorts in LDS), from csrc/"""
    internal, kernels = _src("dvcc_internal.h"), _src("dvcc_kernels.hip")
    assert re.search(r"constexpr\s+int\s+kTile\s*=\s*kBlock\s*\*\s*kIPT\s*;", internal)
    assert re.search(r"constexpr\s+int\s+kBucketIdxBits\s*=\s*32\s*-\s*kBucketHiMax\s*;", kernels)
    assert re.search(r"constexpr\s+uint32_t\s+kBucketCap\s*=\s*1u\s*<<\s*kBucketIdxBits\s*;", kernels)
    mul = int(re.search(r"constexpr\s+uint32_t\s+kRowHashMul\s*=\s*(0x[0-9A-Fa-f]+)u\s*;", internal).group(1), 16)
    max_n = re.search(r"constexpr\s+uint64_t\s+kBucketMaxN\s*=\s*(\d+)u\s*<<\s*(\d+)\s*;", internal)
    hi_max = _const(internal, "kBucketHiMax")
    return dict(kRowHashMul=mul, kRadixBits=_const(internal, "kRadixBits"),
                kRadixMaxBits=_const(internal, "kRadixMaxBits"), kBucketHiMax=hi_max,
                kBucketMaxN=int(max_n.group(1)) << int(max_n.group(2)),
                kTile=_const(internal, "kBlock") * _const(internal, "kIPT"),
                kBucketThreads=int(re.search(r"#define\s+DVCC_BUCKET_THREADS\s+(\d+)", kernels).group(1)),
                kBucketGroup=_const(kernels, "kBucketGroup"), kBucketCap=1 << (32 - hi_max))


K = structural_constants()
MUL = K["kRowHashMul"]
ALL_BITS = tuple(range(1, 33))

# ------------------------------------------------------------- the expected path, by hand
BUCKET_MAX_N = 2 * 2 ** 20
NINE_BIT = (9, 17, 18, 25, 26, 27)
TEN_BIT = (10, 19, 20, 28, 29, 30)
LSD_PASSES = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1, 9: 1, 10: 1,
              11: 2, 12: 2, 13: 2, 14: 2, 15: 2, 16: 2, 17: 2, 18: 2, 19: 2, 20: 2,
              21: 3, 22: 3, 23: 3, 24: 3, 25: 3, 26: 3, 27: 3, 28: 3, 29: 3, 30: 3,
              31: 4, 32: 4}
# the bucket sort's first digit: 8 bits of the hash, 9 at 27 key bits, 10 at 28
BUCKET_LO = {kb: 8 for kb in range(9, 27)}
BUCKET_LO[27] = 9
BUCKET_LO[28] = 10


def expected_path(key_bits, n, on_dev=False, lsd=False):
    """(path, launches, digit width): ("bucket", 2, lo) or ("lsd", passes, w)"""
    if 8 < key_bits <= 28 and not lsd and (on_dev or n <= BUCKET_MAX_N):
        return "bucket", 2, BUCKET_LO[key_bits]
    w = 9 if key_bits in NINE_BIT else 10 if key_bits in TEN_BIT else 8
    return "lsd", LSD_PASSES[key_bits], w


def header_path(key_bits, n, on_dev, lsd, k=None):
    """dvcc_internal.h's radix_digit_bits, radix_passes, kBucketLoBits and
    bucket_sort_applies (hist0_done = false) restated line by line, over the
    constants read from the header"""
    k = k or K
    radix_bits, radix_max_bits, hi_max = k["kRadixBits"], k["kRadixMaxBits"], k["kBucketHiMax"]

    def radix_digit_bits(kb):
        p8 = (kb + radix_bits - 1) // radix_bits
        if p8 < 2:
            return radix_bits
        w = (kb + p8 - 2) // (p8 - 1)
        return w if w <= radix_max_bits else radix_bits

    def radix_passes(kb):
        w = radix_digit_bits(kb)
        return (kb + w - 1) // w

    def bucket_lo_bits(kb):
        return kb - hi_max if kb - hi_max > radix_bits else radix_bits

    def bucket_sort_applies(nn, kb, n_on_dev):
        return kb > radix_bits and kb <= radix_max_bits + hi_max and (n_on_dev or nn <= k["kBucketMaxN"])

    if not lsd and bucket_sort_applies(n, key_bits, on_dev):
        return "bucket", 2, bucket_lo_bits(key_bits)
    return "lsd", radix_passes(key_bits), radix_digit_bits(key_bits)


# ------------------------------------------------------------- the reference
def stable_by(keys, primary):
    return keys[np.argsort(primary, kind="stable")]


def rows_of(keys):
    return keys >> np.uint64(32)


def row_hash(rows, key_bits):
    """h = row * kRowHashMul mod 2^key_bits (rows: uint64 array or int)"""
    if isinstance(rows, np.ndarray):
        return (rows * np.uint64(MUL)) & np.uint64((1 << key_bits) - 1)
    return (rows * MUL) & ((1 << key_bits) - 1)


def primary(keys, key_bits, path):
    return rows_of(keys) if path == "lsd" else row_hash(rows_of(keys), key_bits)


def expected_order(keys, key_bits, path):
    return stable_by(keys, primary(keys, key_bits, path))


def mul_inverse(key_bits):
    """kRowHashMul's inverse mod 2^key_bits (the multiplier is odd)"""
    return pow(MUL, -1, 1 << key_bits)


def unhash(h, key_bits):
    """the row whose hash is h"""
    if isinstance(h, np.ndarray):
        return (h.astype(np.uint64) * np.uint64(mul_inverse(key_bits))) & np.uint64((1 << key_bits) - 1)
    return (h * mul_inverse(key_bits)) & ((1 << key_bits) - 1)


def with_payload(rows):
    """row i << 32 | n - 1 - i"""
    rows = np.asarray(rows, dtype=np.uint64)
    n = len(rows)
    return (rows << np.uint64(32)) | np.arange(n - 1, -1, -1, dtype=np.uint64)


FILLER_PAYLOAD = 0xFFFFFFFF


def filler(key_bits):
    """what lies past a device count: the last row with the largest payload --
    sorted in, it would end every path's output (or its bucket's)"""
    return ((1 << key_bits) - 1) << 32 | FILLER_PAYLOAD


# ------------------------------------------------------------- property checks, whatever the path
def check_row_queues(inp, out):
    """out is a permutation of inp, every row's keys are contiguous and, inside
    a row, in input order (payloads descend with the input position)"""
    assert out.shape == inp.shape
    assert (np.sort(out) == np.sort(inp)).all(), "not a permutation of the input"
    if len(out) < 2:
        return
    r, p = rows_of(out), out & np.uint64(0xFFFFFFFF)
    same = r[1:] == r[:-1]
    assert int((~same).sum()) + 1 == len(np.unique(rows_of(inp))), "a row's keys are not contiguous"
    assert (p[:-1][same] > p[1:][same]).all(), "a row's keys left their input order"


# ------------------------------------------------------------- key sets
SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 3 * 4096 + 1000)
RUN = 65  # a run of equal rows longer than a wave's step


def digit_rows(key_bits, path, width):
    """one row per digit value of every pass: LSD, d << width * p for every
    pass p (the top digit partial); bucket sort, the rows whose hash is
    b << hi_bits (every first-pass bucket) and b0 << hi_bits | d << 8 * p
    (every 8-bit digit of the bits k_bucket_sort sorts by, inside bucket b0)"""
    rows = []
    if path == "lsd":
        for lo in range(0, key_bits, width):
            rows += [d << lo for d in range(1 << min(width, key_bits - lo))]
        return np.array(rows, dtype=np.uint64)
    hi_bits = key_bits - width
    hs = [b << hi_bits for b in range(1 << width)]
    b0 = (1 << width) - 2
    for lo in range(0, hi_bits, 8):
        hs += [b0 << hi_bits | d << lo for d in range(1 << min(8, hi_bits - lo))]
    return unhash(np.array(hs, dtype=np.uint64), key_bits)


KEY_SETS = ("uniform", "row_0", "row_max", "bit0_alternating", "bit0_runs", "top_alternating", "top_runs",
            "descending", "digits")


def key_set(name, key_bits, n, path="lsd", width=8, seed=0):
    """n keys of the named set, rows below 2^key_bits, payload n - 1 - i"""
    top, i = 1 << key_bits, np.arange(n, dtype=np.uint64)
    if name == "uniform":
        rng = np.random.default_rng([seed, key_bits, n])
        rows = rng.integers(0, top, size=n, dtype=np.uint64)
    elif name == "row_0":
        rows = np.zeros(n, dtype=np.uint64)
    elif name == "row_max":
        rows = np.full(n, top - 1, dtype=np.uint64)
    elif name in ("bit0_alternating", "bit0_runs", "top_alternating", "top_runs"):
        # (the larger row first: an unsorted start; key_bits == 1: bit 0 is the top bit)
        a = top - 1
        b = a ^ 1 if name.startswith("bit0") else a ^ (top >> 1)
        pick = i % np.uint64(2) if name.endswith("alternating") else (i // np.uint64(RUN)) % np.uint64(2)
        rows = np.where(pick == 0, np.uint64(a), np.uint64(b))
    elif name == "descending":
        # distinct while n <= 2^key_bits and spread over every digit; wraps above
        step = max(1, top // max(n, 1))
        rows = ((np.uint64(n - 1) - i) * np.uint64(step)) % np.uint64(top)
    elif name == "digits":
        d = digit_rows(key_bits, path, width)[::-1]
        rows = d[i % np.uint64(len(d))]
    else:
        raise KeyError(name)
    return with_payload(rows)


# ------------------------------------------------------------- placed buckets
# (kBucketCap + 1 = 16,385 is also two global chunks of 8,192 keys and one key)
PLACED_M = (1, 2, 511, 512, 513, 8191, 8192, 8193, 16384, 16385, 40000)
assert 2 * 8192 + 1 in PLACED_M
PLACED_HI_BITS = (1, 8, 9, 16, 17, 18)
# (key_bits, lo): every hi_bits at lo = 8; lo = 9 and 10 exist at 27 and 28 key bits only (hi_bits 18)
PLACED_WIDTHS = tuple((8 + hb, 8) for hb in PLACED_HI_BITS) + ((27, 9), (28, 10))


def placed_low(m, hi_bits, pattern):
    """m low-hash values: "descending" from the largest, cyclically (every
    value of the hi_bits repeats once m exceeds 2^hi_bits); "pairs": the same
    with every value twice in a row (a step's lanes share digits two by two in
    the first pass); "few_rows": 37 random values drawn at random, so every
    digit of every pass repeats inside a step at random lanes and no two passes
    can undo each other's mistakes; "equal": one row"""
    size = 1 << hi_bits
    if pattern == "equal":
        return np.full(m, size - 1 if hi_bits > 1 else 1, dtype=np.uint64)
    if pattern == "few_rows":
        rng = np.random.default_rng([m, hi_bits])
        return rng.choice(rng.integers(0, size, size=37, dtype=np.uint64), size=m)
    i = np.arange(m, dtype=np.uint64)
    if pattern == "pairs":
        i = i // np.uint64(2)
    else:
        assert pattern == "descending"
    return (np.uint64(size - 1) - i % np.uint64(size)).astype(np.uint64)


PLACED_PATTERNS = ("descending", "pairs", "few_rows", "equal")


def placed_rows(key_bits, lo, b, low):
    """the rows whose hash is b << hi_bits | low: all in first-pass bucket b"""
    hi_bits = key_bits - lo
    assert 0 <= b < 1 << lo and (np.asarray(low) < 1 << hi_bits).all()
    return unhash(np.uint64(b << hi_bits) | np.asarray(low, dtype=np.uint64), key_bits)


def placed_bucket(key_bits, lo, buckets):
    """keys of [(b, m, pattern), ...] in that input order, nothing elsewhere"""
    rows = [placed_rows(key_bits, lo, b, placed_low(m, key_bits - lo, pat)) for b, m, pat in buckets]
    return with_payload(np.concatenate(rows))
