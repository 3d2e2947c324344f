// index_math_test.cpp -- the index probe's arithmetic
// (deneva-plus_amd/csrc/dvcc_index_math.h) against exact unsigned __int128
// division, on the host: div_magic / divmod_magic give the exact quotient and
// remainder with at most two corrections, and key_split's bucket and tag are
// the bucket function's and key_tag's.  Built with the address and
// undefined-behaviour sanitizers by tests/test_index_cases_cpu.py; prints
// "ok <checks> corrections <the most any division took>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dvcc_index_math.h"

using u64 = uint64_t;
using u128 = unsigned __int128;

namespace {
struct Desc {  // what key_split reads of a table descriptor
    uint32_t hash_kind, part_cnt;
    u64 nbuckets, m_part, m_nb;
};

u64 checks = 0, max_corrections = 0;

[[noreturn]] void fail(const char *what, u64 n, u64 d, u64 d2) {
    std::printf("FAIL %s n=%llu d=%llu d2=%llu\n", what, (unsigned long long)n, (unsigned long long)d,
                (unsigned long long)d2);
    std::exit(1);
}

void check_div(u64 n, u64 d) {
    const u64 m = dvcc::div_magic(d);
    if (m != (u64)((((u128)1 << 64) - 1) / d)) fail("div_magic", n, d, 0);
    u64 r = ~0ull;
    const u64 q = dvcc::divmod_magic(n, d, m, r);
    const u64 qe = (u64)((u128)n / d), re = (u64)((u128)n % d);
    if (q != qe || r != re) fail("divmod_magic", n, d, 0);
    const u64 est = dvcc::mulhi64(n, m);  // what the corrections start from
    if (est > qe || qe - est > 2) fail("corrections", n, d, 0);
    if (qe - est > max_corrections) max_corrections = qe - est;
    checks++;
}

// key_split of a table of nb buckets (P partitions under DV_HASH_YCSB)
void check_split(uint32_t kind, u64 nb, uint32_t P, u64 key) {
    const Desc t{kind, P, nb, dvcc::div_magic(P), dvcc::div_magic(nb)};
    uint32_t tag = ~0u;
    const u64 bk = dvcc::key_split(t, key, tag);
    const u64 be = kind == DV_HASH_YCSB ? (u64)(((u128)key / P) % nb) : (u64)((u128)key % nb);
    const u64 qe = kind == DV_HASH_YCSB ? (u64)((u128)key / P / nb) : (u64)((u128)key / nb);
    const u128 code = kind == DV_HASH_YCSB ? (u128)qe * P + key % P : (u128)qe;
    const uint32_t te = qe >= dvcc::kTagWide || code >= dvcc::kTagWide ? dvcc::kTagWide : (uint32_t)code;
    if (bk != be) fail("bucket", key, nb, P);
    if (tag != te || tag != dvcc::key_tag(kind, nb, P, key)) fail("tag", key, nb, P);
    checks++;
}

u64 splitmix(u64 &s) {
    u64 z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// 0, d - 1, d, d + 1, the multiples of d nearest 2^32, 2^63 and 2^64 with
// their neighbours, 2^64 - 1, and a seeded sample of every magnitude
std::vector<u64> dividends(u64 d, u64 seed) {
    std::vector<u64> v = {0, d - 1, d, d + 1, ~0ull};
    const u128 at[3] = {(u128)1 << 32, (u128)1 << 63, (u128)1 << 64};
    for (const u128 p : at) {
        const u128 below = p / d * d;  // the nearest multiples on either side
        for (const u128 mult : {below, below + d})
            for (int e = -1; e <= 1; e++) {
                if (mult == 0 && e < 0) continue;
                const u128 n = mult + e;
                if (n >> 64) continue;
                v.push_back((u64)n);
            }
    }
    u64 s = seed;
    for (int i = 0; i < 4096; i++) {
        const u64 x = splitmix(s);
        v.push_back(x >> (splitmix(s) & 63));
    }
    return v;
}
}  // namespace

int main() {
    const u64 ds[] = {1, 2, 3, 7, 33, 97, 300, 1021, (1ull << 31) - 1, (1ull << 32) + 1};
    for (const u64 d : ds)
        for (const u64 n : dividends(d, d)) check_div(n, d);
    // key_split: every d as a bucket count, alone (DV_HASH_MOD) and behind
    // every partition count that fits 32 bits (DV_HASH_YCSB)
    for (const u64 nb : ds)
        for (const u64 n : dividends(nb, nb ^ 0x5555)) {
            check_split(DV_HASH_MOD, nb, 1, n);
            for (const u64 P : ds) {
                if (P >> 32) continue;
                check_split(DV_HASH_YCSB, nb, (uint32_t)P, n);
                // ... and keys whose quotient by P is an edge of nb
                if (!(((u128)n * P) >> 64)) check_split(DV_HASH_YCSB, nb, (uint32_t)P, n * P + (P - 1));
            }
        }
    std::printf("ok %llu corrections %llu\n", (unsigned long long)checks, (unsigned long long)max_corrections);
    return 0;
}
