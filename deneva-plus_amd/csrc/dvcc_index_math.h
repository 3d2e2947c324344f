// dvcc_index_math.h -- the index probe's arithmetic: the key tag of an
// implicit-row direct map and the division-free bucket function (key_split,
// dvcc_internal.h).  Host-compilable: <cstdint> and dvcc.h alone, so a host
// program can hold it to exact 128-bit division (tests/cpp/index_math_test.cpp).
// On the device the multiply-high is __umul64hi, on the host a 128-bit product.
#pragma once
#include <cstdint>

#include "dvcc.h"

#if defined(__HIPCC__)
#define DVCC_HD __host__ __device__
#define DVCC_HD_INLINE __host__ __device__ __forceinline__
#else
#define DVCC_HD
#define DVCC_HD_INLINE inline
#endif

namespace dvcc {

// Key tag of an implicit-row direct map.  A bucket's keys differ only in
// what the bucket function drops: with DV_HASH_YCSB, b = (k / P) % nb, a key
// is (q, b, lo) with q = k / P / nb and lo = k % P; with DV_HASH_MOD,
// b = k % nb, it is (q, b).  So q * P + lo (P = 1 for MOD) names the key
// within its bucket exactly; a loaded row stores it in one byte when it is
// below kTagWide (YCSB's loader: q = 0, the tag is the partition id), else
// kTagWide, and a probe compares tags -- equal tags below kTagWide mean equal
// keys, unequal ones a missing key -- reading the 8-byte pkey only for
// kTagWide.  Config D's probe target shrinks from 134 MB to 16.8 MB.
constexpr uint32_t kTagWide = 255;
DVCC_HD inline uint8_t key_tag(uint32_t hash_kind, uint64_t nbuckets, uint32_t part_cnt, uint64_t key) {
    const uint64_t P = hash_kind == DV_HASH_YCSB ? part_cnt : 1u;
    const uint64_t q = key / P / nbuckets;
    if (q >= kTagWide) return (uint8_t)kTagWide;
    const uint64_t code = q * P + key % P;
    return (uint8_t)(code < kTagWide ? code : kTagWide);
}
// the high 64 bits of a * b
DVCC_HD_INLINE uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// n / d and n % d for every 64-bit n without a division: m = div_magic(d) =
// floor((2^64 - 1) / d) puts mulhi(n, m) within 2 below the quotient
DVCC_HD inline uint64_t div_magic(uint64_t d) { return d ? ~0ull / d : 0ull; }
DVCC_HD_INLINE uint64_t divmod_magic(uint64_t n, uint64_t d, uint64_t m, uint64_t &r) {
    uint64_t q = mulhi64(n, m);
    r = n - q * d;
    if (r >= d) { q++; r -= d; }
    if (r >= d) { q++; r -= d; }
    return q;
}
// the bucket of `key` and its key tag (key_tag) in one pass.  Desc: the
// table's descriptor (TableDesc, dvcc_internal.h) -- hash_kind, part_cnt,
// nbuckets and m_part / m_nb, the div_magic of part_cnt / nbuckets
template <class Desc>
DVCC_HD_INLINE uint64_t key_split(const Desc &t, uint64_t key, uint32_t &tag) {
    uint64_t lo = 0, bk = 0, q;
    if (t.hash_kind == DV_HASH_YCSB) {
        const uint64_t q1 = divmod_magic(key, t.part_cnt, t.m_part, lo);
        q = divmod_magic(q1, t.nbuckets, t.m_nb, bk);
        const uint64_t code = q * t.part_cnt + lo;
        tag = q >= kTagWide || code >= kTagWide ? kTagWide : (uint32_t)code;
    } else {
        q = divmod_magic(key, t.nbuckets, t.m_nb, bk);
        tag = q >= kTagWide ? kTagWide : (uint32_t)q;
    }
    return bk;
}

}  // namespace dvcc
