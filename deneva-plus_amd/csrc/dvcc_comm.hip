// dvcc_comm.hip -- partitioned epochs driven from the engine over RCCL
// (SURVEY.md 8(b) dv_comm_init, 8(e)).
//
// One process per GPU; rank r owns partition r (PART_CNT == ranks,
// GET_NODE_ID(part) == part, system/global.h:294).  dv_epoch_run_part runs a
// whole epoch from this rank's client batch:
//   1. split the batch by owner rank = key % PART_CNT (YCSBWorkload::
//      key_to_part, benchmarks/ycsb_wl.cpp:69-74) on the device, stably, into
//      16-byte dv_access records;
//   2. one all-to-all of the counts and one all-to-allv of the records -- the
//      RQRY messages of msg_queue / nanomsg (ycsb_txn.cpp:160-175,
//      transport/transport.cpp:224-304).  Records arrive in origin-rank order,
//      which is the global sequence order (epoch, origin node, position) Calvin
//      locks in (work_queue.cpp:105-151);
//   3. NO_WAIT / WAIT_DIE / OCC: decision rounds, each closed by an
//      all-reduce(MAX) of the verdict bytes of the still-undecided txns in list
//      order -- TxnManager::received_response's vote combine (txn.cpp:544-554)
//      for every open txn at once -- queued two rounds ahead of the outcome the
//      host reads, each all-reduce sized by the list length of two rounds
//      earlier (the same number on every rank); CALVIN needs no votes;
//   4. execute the committed accesses on this rank's rows.
// Everything runs on the context's stream, RCCL collectives included.  The
// Python driver (deneva-plus_amd/dvcc/partitioned.py) runs the same protocol
// over torch.distributed.
#include <rccl/rccl.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <cstring>
#include <thread>
#include <vector>

#include "dvcc_common.h"

namespace dvcc {

// flags word of the argument vote (element-wise MAX across ranks)
constexpr uint32_t kVoteBadArg = 1u, kVoteOverflow = 2u;

// ---- owner split: per-block owner counts, then a stable scatter of records.
// The owner of an access is key % PART_CNT (YCSB), or the caller's per-access
// owner byte (TPC-C: the warehouse's partition, wh_to_part,
// tpcc_helper.cpp:161-164); an owner byte >= PART_CNT is an argument error,
// voted like the others (xvote[1]) -- the access counts as rank 0's meanwhile.
__device__ __forceinline__ uint32_t owner_of(const uint64_t *keys, const uint8_t *own, uint64_t i, uint32_t P,
                                             uint32_t *bad) {
    if (!own) return (uint32_t)(keys[i] % P);
    const uint32_t o = own[i];
    if (o < P) return o;
    atomicOr(bad, kVoteBadArg);
    return 0u;
}

__global__ __launch_bounds__(kBlock) void k_owner_count(const uint64_t *__restrict__ keys,
                                                        const uint8_t *__restrict__ own, uint64_t n,
                                                        uint32_t P, uint32_t *__restrict__ counts,
                                                        uint32_t nb, uint32_t *xvote) {
    __shared__ uint32_t c[kRadix];
    for (uint32_t o = threadIdx.x; o < kRadix; o += kBlock) c[o] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    for (uint32_t j = threadIdx.x; j < (uint32_t)kTile; j += kBlock)
        if (base + j < n) atomicAdd(&c[owner_of(keys, own, base + j, P, &xvote[1])], 1u);
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < P; o += kBlock) counts[(uint64_t)o * nb + blockIdx.x] = c[o];
}

// counts[o][b] -> exclusive prefix within owner o; tot[o] = owner o's total
__global__ __launch_bounds__(kBlock) void k_owner_scan(uint32_t *__restrict__ counts, uint32_t nb,
                                                       uint32_t *__restrict__ tot) {
    __shared__ uint32_t lds4[4];
    uint32_t *c = counts + (uint64_t)blockIdx.x * nb;
    const uint32_t t = block_chunk_scan256(c, nb, lds4);
    if (threadIdx.x == 0) tot[blockIdx.x] = t;
}

// A batch's txn id at or past txns_per_rank would become another origin's
// global id (rank * tpr + id) and merge two txns: it is sent as an id past
// every epoch (kBadTxn), which the decider's probe rejects (ERRB_TXN, an
// input error voted out on every rank before anything executes).
constexpr uint32_t kBadTxn = 0xFFFFFFFFu;
// (origin-major: stride 1, base rank * tpr; position-major: stride P, base rank)
__device__ __forceinline__ uint32_t global_txn(uint32_t t, uint32_t tpr, uint32_t base, uint32_t stride = 1) {
    return t < tpr ? t * stride + base : kBadTxn;
}

// record i of the batch -> its owner's segment, in batch order (stable: a
// wave walks 64 consecutive records per step, ranks by ballot); TPC-C
// records carry their table, and their operation words go the same way into
// args_out
__global__ __launch_bounds__(kBlock) void k_owner_scatter(const uint64_t *__restrict__ keys,
                                                          const uint8_t *__restrict__ types,
                                                          const uint32_t *__restrict__ acc_txn,
                                                          const uint8_t *__restrict__ own,
                                                          const uint8_t *__restrict__ tables,
                                                          const uint64_t *__restrict__ args,
                                                          uint64_t n, uint32_t P, uint32_t tpr, uint32_t txn_base,
                                                          uint32_t txn_stride, const uint32_t *__restrict__ counts,
                                                          const uint32_t *__restrict__ tot, uint32_t nb,
                                                          dv_access *__restrict__ out,
                                                          uint64_t *__restrict__ args_out, uint32_t *xvote) {
    __shared__ uint32_t wc[4][kRadix];
    __shared__ uint32_t obase[kRadix];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t o = 0; o < P; o++) {
            obase[o] = s;
            s += tot[o];
        }
    }
    for (uint32_t o = tid; o < kRadix; o += kBlock) wc[0][o] = wc[1][o] = wc[2][o] = wc[3][o] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kTile + wave * (64 * kIPT);
    uint32_t own_[kIPT], r[kIPT];
    for (int j = 0; j < kIPT; j++) {
        const uint64_t idx = base + j * 64 + lane;
        const bool valid = idx < n;
        const uint32_t o = valid ? owner_of(keys, own, idx, P, &xvote[1]) : 0u;
        const uint64_t peers = match_digit(o, __ballot(valid));
        const uint32_t before = wc[wave][o];
        own_[j] = o;
        r[j] = before + mask_rank(peers);
        if (valid && lane == (uint32_t)__builtin_ctzll(peers)) wc[wave][o] = before + (uint32_t)__popcll(peers);
    }
    __syncthreads();
    for (int j = 0; j < kIPT; j++) {
        const uint64_t idx = base + j * 64 + lane;
        if (idx >= n) continue;
        const uint32_t o = own_[j];
        uint32_t wpre = 0;
        for (uint32_t w = 0; w < wave; w++) wpre += wc[w][o];
        const uint64_t dst = (uint64_t)obase[o] + counts[(uint64_t)o * nb + blockIdx.x] + wpre + r[j];
        dv_access a;
        a.key = keys[idx];
        a.txn_seq = global_txn(acc_txn[idx], tpr, txn_base, txn_stride);  // (an id past tpr: rejected by the probe)
        a.type = types[idx];
        a.table = tables ? tables[idx] : 0;
        a.flags = 0;
        out[dst] = a;
        if (args_out) args_out[dst] = args[idx];
    }
}

// the received record count exceeds this context's capacity: a vote, so every
// rank leaves together (xvote[1] |= kVoteOverflow)
__global__ void k_recv_check(const uint64_t *__restrict__ recvc, uint32_t P, uint64_t cap,
                             uint32_t *__restrict__ xvote) {
    if (threadIdx.x != 0) return;
    uint64_t n = 0;
    for (uint32_t o = 0; o < P; o++) n += recvc[o];
    if (n > cap) xvote[1] |= kVoteOverflow;
}

// ---- replicated epochs (run_part): every rank receives the whole epoch's
// access list in the global order -- the batches of ranks 0..P-1, which is
// Calvin's sequence (work_queue.cpp:105-151) -- decides it alone, and
// executes its own rows.  Per access 9 bytes travel: the key as a 32-bit row
// id (a key is the row of the global row space, which fits 31 bits; a wider
// key saturates and fails the probe like any key no partition holds), the
// txn id made global by its sender, and the type -- three all-gathers into
// contiguous arrays that are the epoch's own inputs (no unpacking).
constexpr uint32_t kRepBlockOff = 2u;

// unequal batches: the gathered parts (rank q's at q * hmax) packed together
__global__ __launch_bounds__(kBlock) void k_rep_compact(const uint32_t *__restrict__ gk,
                                                        const uint32_t *__restrict__ gt,
                                                        const uint8_t *__restrict__ gy, uint64_t hmax,
                                                        const uint64_t *__restrict__ cnt, uint32_t P,
                                                        uint32_t *__restrict__ k32, uint32_t *__restrict__ t32,
                                                        uint8_t *__restrict__ ty) {
    for (uint32_t r = blockIdx.y; r < P; r += gridDim.y) {
        uint64_t off = 0;
        for (uint32_t q = 0; q < r; q++) off += cnt[q];
        const uint64_t n = cnt[r] < hmax ? cnt[r] : hmax, src = (uint64_t)r * hmax;
        for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
            k32[off + i] = gk[src + i];
            t32[off + i] = gt[src + i];
            if (gy) ty[off + i] = gy[src + i];  // (position-major: the write bit rides in the row ids)
        }
    }
}

// epoch groups: row id | wr << 31 and the global txn id, 8 B per access
// (txn t of this origin is t * stride + txn_base: origin-major stride 1, base
// rank * tpr; position-major stride P, base rank)
__global__ __launch_bounds__(kBlock) void k_group_pack(const uint64_t *__restrict__ keys,
                                                       const uint8_t *__restrict__ types,
                                                       const uint32_t *__restrict__ txn, uint64_t n,
                                                       uint32_t tpr, uint32_t stride, uint32_t txn_base,
                                                       uint32_t *__restrict__ k32, uint32_t *__restrict__ t32) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t k = keys[i];
        // a key past 31 bits saturates and fails the decider's range check
        k32[i] = ((k >> 31) ? 0x7FFFFFFFu : (uint32_t)k) | (types[i] == DV_WR ? 0x80000000u : 0u);
        const uint32_t t = txn[i];
        t32[i] = t < tpr ? t * stride + txn_base : kBadTxn;
    }
}

// Compact batches (epoch groups whose global row space P x rows is below
// 2^30, P <= kXMaxP): 4 B per access -- row id | start << 30 | wr << 31,
// start = the first access of its txn -- in place of the 8 B above (half the
// all-to-allv bytes over xGMI); the decider numbers the txns again from the
// starts (k_group_txn_count, k_group_txn_ids).  That needs dense txn ids (0
// first, then +0 or +1 per access, below n_txn): anything else sets *bad, and
// the outcome vote fails the group on every rank before anything executes.
constexpr uint32_t GP_START = 1u << 30;
constexpr uint32_t kXMaxP = 64;
// (every batch of the group in one launch: blockIdx.y = epoch)
struct PackSrc {
    const uint64_t *keys[kXMaxP];
    const uint8_t *types[kXMaxP];
    const uint32_t *recs[kXMaxP];  // (optional: dv_epoch_dev::recs32, read instead of keys + types)
    const uint32_t *txn[kXMaxP];
    uint64_t n[kXMaxP], off[kXMaxP];
    uint32_t n_txn[kXMaxP];
};
__global__ __launch_bounds__(kBlock) void k_group_pack_c(PackSrc src, uint32_t *__restrict__ k32_all,
                                                         uint32_t *__restrict__ bad, int tbx) {
    const uint32_t e = blockIdx.y;
    const uint64_t *__restrict__ keys = src.keys[e];
    const uint8_t *__restrict__ types = src.types[e];
    const uint32_t *__restrict__ recs = src.recs[e];
    const uint32_t *__restrict__ txn = src.txn[e];
    const uint64_t n = src.n[e];
    const uint32_t n_txn = src.n_txn[e];
    uint32_t *__restrict__ k32 = k32_all + src.off[e];
    bool b = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        uint64_t k;
        bool wr;
        if (recs) {  // (4 bytes per access instead of 9)
            const uint32_t r = recs[i];
            k = r & 0x7FFFFFFFu;
            wr = (r >> 31) != 0;
        } else {
            k = keys[i];
            wr = types[i] == DV_WR;
        }
        bool start = false;
        if (!tbx) {  // (tbx: the batch's txn_begin travels beside it)
            const uint32_t t = txn[i];
            const uint32_t pt = i ? txn[i - 1] : 0u;
            start = i == 0 || t != pt;
            if (t >= n_txn || (i == 0 ? t != 0u : (t != pt && t != pt + 1u))) b = true;
        }
        // (a key past 30 bits saturates and fails the decider's range check)
        k32[i] = ((k >> 30) ? 0x3FFFFFFFu : (uint32_t)k) | (start ? GP_START : 0u) | (wr ? 0x80000000u : 0u);
    }
    if (b) atomicOr(bad, 1u);
}

// the received compact batches: origin q's accesses at [eoff[q], eoff[q+1]),
// cut into tiles of kXTile that never span two origins (origin q's tiles
// from toff[q])
constexpr int kXIPT = 16;
constexpr uint32_t kXTile = kBlock * kXIPT;
struct XSegs {
    uint32_t P, tpr;
    uint64_t mP, mT;  // div_magic(P), div_magic(tpr): position-major index arithmetic
    uint64_t eoff[kXMaxP + 1];
    uint32_t toff[kXMaxP + 1];
    // tbx: the words of origin q's txn_begin that landed at q * (tpr + 1) (its
    // n_txn + 1, or 0 for a batch without txns); the later entries stand for
    // the segment's end
    uint32_t tbw[kXMaxP];
};
__device__ __forceinline__ uint32_t xseg_of(const XSegs &s, uint32_t tile) {
    uint32_t q = 0;
    while (q + 1 < s.P && s.toff[q + 1] <= tile) q++;  // (origins without accesses hold no tile)
    return q;
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *red) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_incl_sum(v, lane);
    if (lane == 63) red[wave] = v;
    __syncthreads();
    const uint32_t t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}

// txn starts per tile (and, position-major, the origins' txn counts zeroed
// for k_group_txn_ids)
__global__ __launch_bounds__(kBlock) void k_group_txn_count(const uint32_t *__restrict__ rk, XSegs s,
                                                            uint32_t *__restrict__ cnt, uint32_t *__restrict__ ncnt) {
    __shared__ uint32_t red[kBlock / 64];
    const uint32_t tile = blockIdx.x, q = xseg_of(s, tile);
    if (ncnt && tile == 0 && threadIdx.x < s.P) ncnt[threadIdx.x] = 0;
    const uint64_t b0 = s.eoff[q] + (uint64_t)(tile - s.toff[q]) * kXTile;
    const uint64_t e = b0 + kXTile < s.eoff[q + 1] ? b0 + kXTile : s.eoff[q + 1];
    uint32_t c = 0;
    for (uint64_t i = b0 + threadIdx.x; i < e; i += kBlock) c += (rk[i] & GP_START) ? 1u : 0u;
    c = block_sum(c, red);
    if (threadIdx.x == 0) cnt[tile] = c;
}

// global txn id of every access (origin q's txn j is q * tpr + j, the id
// dv_epoch_group_run gives it; position-major, tbo non-null: the origin-local
// j, and each txn's first access within its origin's segment into tbo, the
// origin's txn count into ncnt -- k_il_begin) into rt, the start bits cleared
// from rk (position-major: left for k_il_move, which copies rk anyway)
__global__ __launch_bounds__(kBlock) void k_group_txn_ids(uint32_t *__restrict__ rk, XSegs s,
                                                          const uint32_t *__restrict__ cnt, uint32_t *__restrict__ rt,
                                                          uint32_t *__restrict__ tbo, uint32_t *__restrict__ ncnt) {
    __shared__ uint32_t red[kBlock / 64], wt[2][kBlock / 64];
    const uint32_t tile = blockIdx.x, q = xseg_of(s, tile);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t b0 = s.eoff[q] + (uint64_t)(tile - s.toff[q]) * kXTile;
    const uint64_t e = b0 + kXTile < s.eoff[q + 1] ? b0 + kXTile : s.eoff[q + 1];
    uint32_t pre = 0;  // the starts of this origin's earlier tiles
    for (uint32_t k = s.toff[q] + threadIdx.x; k < tile; k += kBlock) pre += cnt[k];
    uint32_t run = block_sum(pre, red);  // (origin-local txn numbers)
    for (uint32_t u = 0; u < (uint32_t)kXIPT; u++) {  // 256 consecutive accesses per step
        const uint64_t i = b0 + (uint64_t)u * kBlock + threadIdx.x;
        const uint32_t w = i < e ? rk[i] : 0u;
        const bool f = (w & GP_START) != 0;
        const uint64_t m = __ballot(f);
        const uint32_t p = u & 1u;
        if (lane == 0) wt[p][wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t base = run;
        for (uint32_t v = 0; v < wave; v++) base += wt[p][v];
        const uint32_t incl = base + (uint32_t)__popcll(m & ((2ull << lane) - 1ull));
        if (i < e) {
            const uint32_t j = incl - 1u;  // (a batch with more txns than tpr fails the pack's check)
            if (!tbo) rk[i] = w & ~GP_START;  // (position-major: k_il_move clears it on the way)
            if (tbo) {
                rt[i] = j;
                if (f && j < s.tpr) tbo[(uint64_t)q * (s.tpr + 1) + j] = (uint32_t)(i - s.eoff[q]);
                if (i + 1 == s.eoff[q + 1]) ncnt[q] = j < s.tpr ? j + 1 : s.tpr;
            } else {
                rt[i] = q * s.tpr + j;
            }
        }
        run += wt[p][0] + wt[p][1] + wt[p][2] + wt[p][3];
    }
}

// ---- position-major epochs (DV_COMM_POSITION_ORDER; not CALVIN, whose
// order is the sequencer's origin by origin): origin q's txn j is sequence
// number j * P + q -- the origins' batches interleaved txn by txn, as
// clients arriving together -- so the decider's prefix (its first n / 32
// txns) holds every origin's first txns and kills in every partition, where
// origin-major it holds origin 0's only.  The batches land contiguous per
// origin; tbo[q * (tpr + 1) + j] is txn j's first access inside origin q's
// segment, ncnt[q] entries valid (later j: the segment's end).
// ncnt null: tbx, the senders' own boundaries (XSegs::tbw entries landed)
__device__ __forceinline__ uint32_t il_start(const XSegs &s, const uint32_t *__restrict__ tbo,
                                             const uint32_t *__restrict__ ncnt, uint32_t q, uint32_t j) {
    return j < (ncnt ? ncnt[q] : s.tbw[q]) ? tbo[(uint64_t)q * (s.tpr + 1) + j]
                                           : (uint32_t)(s.eoff[q + 1] - s.eoff[q]);
}

// tbx: the receiver checks each landed batch's boundaries -- 0 first, rising,
// its access count last -- in the launch that reads them (k_tb_origin,
// k_il_begin).  Txn j < tpr of origin q checks entry j against entry j + 1;
// a batch of tpr = 0 txns is checked at the epoch's end entry (tbx_bad_end).
__device__ __forceinline__ bool tbx_bad(const XSegs &s, const uint32_t *__restrict__ tbr, uint32_t q, uint32_t j) {
    const uint32_t w = s.tbw[q], seg = (uint32_t)(s.eoff[q + 1] - s.eoff[q]);
    if (w == 0) return j == 0 && seg != 0u;  // (no boundaries: an empty batch only)
    const uint32_t nt = w - 1u;
    if (j > nt) return false;
    const uint32_t *tq = tbr + (uint64_t)q * (s.tpr + 1);
    const uint32_t v = tq[j];
    if (j == 0 && v != 0u) return true;
    if (j == nt) return v != seg;
    return v > tq[j + 1] || (j + 1 == nt && tq[nt] != seg);
}
__device__ __forceinline__ bool tbx_bad_end(const XSegs &s, const uint32_t *__restrict__ tbr) {
    bool b = false;
    if (s.tpr == 0)
        for (uint32_t q = 0; q < s.P; q++) b |= tbx_bad(s, tbr, q, 0);
    return b;
}

// wide batches (the senders' ids): tbo by a lower bound over each segment's
// ids, sorted in a well-formed batch (k_il_move checks what it moves)
__global__ __launch_bounds__(kBlock) void k_il_bounds(const uint32_t *__restrict__ rt, XSegs s,
                                                      uint32_t *__restrict__ tbo, uint32_t *__restrict__ ncnt) {
    const uint64_t n = (uint64_t)s.P * (s.tpr + 1);
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kBlock) {
        const uint32_t q = (uint32_t)(x / (s.tpr + 1)), j = (uint32_t)(x % (s.tpr + 1));
        const uint64_t t = (uint64_t)j * s.P + q;  // (j == tpr: past every id of the segment)
        uint64_t lo = s.eoff[q], hi = s.eoff[q + 1];
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((uint64_t)rt[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        tbo[x] = (uint32_t)(lo - s.eoff[q]);
        if (j == 0) ncnt[q] = s.tpr + 1;
    }
}

// tb[t]: where sequence number t = j * P + q starts in the interleaved epoch
// -- after txns 0..j of origins 0..q-1 and txns 0..j-1 of origins q..P-1 --
// which is the decider's txn_begin (tb[P * tpr] = every access), and shift
// [q * tpr + j] = tb[t] minus the txn's first access inside its segment (the
// move's one lookup per access)
__global__ __launch_bounds__(kBlock) void k_il_begin(XSegs s, const uint32_t *__restrict__ tbo,
                                                     const uint32_t *__restrict__ ncnt, uint32_t *__restrict__ tb,
                                                     uint32_t *__restrict__ shift, uint32_t *__restrict__ bad) {
    const uint32_t n = s.P * s.tpr;
    bool b = false;
    for (uint32_t t = blockIdx.x * kBlock + threadIdx.x; t <= n; t += gridDim.x * kBlock) {
        uint64_t qq = 0;
        const uint32_t j = (uint32_t)divmod_magic(t, s.P, s.mP, qq), q = (uint32_t)qq;
        uint32_t d = 0, own = 0;
        for (uint32_t o = 0; o < s.P; o++) {
            const uint32_t st = il_start(s, tbo, ncnt, o, o < q ? j + 1 : j);
            d += st;
            if (o == q) own = st;
        }
        tb[t] = d;
        if (t < n) shift[(uint64_t)q * s.tpr + j] = d - own;
        if (bad) b |= t < n ? tbx_bad(s, tbo, q, j) : tbx_bad_end(s, tbo);  // (tbx: the landed boundaries)
    }
    if (b) atomicOr(bad, 1u);
}

// every landed access to its place in the interleaved epoch (tiles of one
// origin, as k_group_txn_ids): position i of origin q's segment goes to
// (i - eoff[q]) + shift of its txn.  WIDE (the senders' ids in rt): an id that
// is not this origin's, past the epoch, or out of order (a malformed batch) is
// not moved and fails the group (*bad, voted with the outcome: DV_ERR_ARG on
// every rank); every store stays inside its txn's [tb[t], tb[t + 1]) and below
// n_acc.  ot (NULL when the decider reads the boundaries only, tb mode): the
// sequence number per access.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_il_move(const uint32_t *__restrict__ rk, const uint32_t *__restrict__ rt,
                                                    XSegs s, const uint32_t *__restrict__ shift,
                                                    const uint32_t *__restrict__ tb, uint64_t n_acc,
                                                    uint32_t *__restrict__ ok, uint32_t *__restrict__ ot,
                                                    uint32_t *__restrict__ bad) {
    const uint32_t tile = blockIdx.x, q = xseg_of(s, tile);
    const uint64_t b0 = s.eoff[q] + (uint64_t)(tile - s.toff[q]) * kXTile;
    const uint64_t e = b0 + kXTile < s.eoff[q + 1] ? b0 + kXTile : s.eoff[q + 1];
    const uint32_t n = s.P * s.tpr;
    bool b = false;
#pragma unroll 4
    for (uint64_t i = b0 + threadIdx.x; i < e; i += kBlock) {
        const uint32_t v = rt[i];
        uint32_t j = v, t = 0;
        bool good = true;
        if (WIDE) {
            uint64_t qq = 0;
            j = (uint32_t)divmod_magic(v, s.P, s.mP, qq);
            good = v < n && (uint32_t)qq == q && (i == s.eoff[q] || rt[i - 1] <= v);
            t = v;
        } else {
            good = j < s.tpr;  // (a batch with too many txns: the pack's check fails the group)
            t = j * s.P + q;
        }
        if (good) {
            const uint64_t d = (i - s.eoff[q]) + shift[(uint64_t)q * s.tpr + j];
            good = d < n_acc && (!WIDE || (d >= tb[t] && d < tb[t + 1]));
            if (good) {
                ok[d] = rk[i] & ~(WIDE ? 0u : GP_START);
                if (ot) ot[d] = t;
            }
        }
        b |= !good;
    }
    if (b) atomicOr(bad, 1u);
}

// ---- epoch groups whose batches bring their txn boundaries (every rank's
// homes carry dv_epoch_dev::txn_begin and the decider takes tb mode; the
// vote's "tbx"): each batch's txn_begin travels beside its rows, straight from
// the caller's buffer (n_txn + 1 words, landing at q * (tpr + 1); XSegs::tbw),
// so the decider needs no start bits, no renumbering and no per-access txn
// ids.  The receiver checks every landed batch (tbx_bad: 0 first, rising, its
// access count last) in the launch that reads it: a bad one fails the group
// (*bad, DV_ERR_ARG on every rank).

// origin-major: the decider's txn_begin -- origin q's txn j at q * tpr + j
// starts at eoff[q] + its offset in q's batch; tb[P * tpr] = every access.
// Each landed batch's boundaries are checked here (tbx_bad): a bad one fails
// the group (*bad, DV_ERR_ARG on every rank); the decider's own range checks
// keep it inside the epoch meanwhile
__global__ __launch_bounds__(kBlock) void k_tb_origin(XSegs s, const uint32_t *__restrict__ tbr,
                                                      uint32_t *__restrict__ tb, uint32_t *__restrict__ bad) {
    const uint64_t n = (uint64_t)s.P * s.tpr;
    bool b = false;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t <= n; t += (uint64_t)gridDim.x * kBlock) {
        if (t == n) {
            tb[t] = (uint32_t)s.eoff[s.P];
            b |= tbx_bad_end(s, tbr);
            continue;
        }
        uint64_t j = 0;
        const uint64_t q = divmod_magic(t, s.tpr, s.mT, j);
        tb[t] = (uint32_t)(s.eoff[q] + il_start(s, tbr, nullptr, (uint32_t)q, (uint32_t)j));
        b |= tbx_bad(s, tbr, (uint32_t)q, (uint32_t)j);
    }
    if (b) atomicOr(bad, 1u);
}

// position-major with the boundaries (no per-access ids): a block per origin
// and tile of kIlTxns txns stages their starts and shifts in LDS and each
// txn's index over its accesses (a byte per access, runs of up to kIlOwn
// accesses; a longer run finds its txns by a binary search of the starts),
// then moves the tile's accesses, one per thread
constexpr uint32_t kIlTxns = 256, kIlOwn = 8192;
__global__ __launch_bounds__(kBlock) void k_il_move_tb(const uint32_t *__restrict__ rk, XSegs s,
                                                       const uint32_t *__restrict__ tbo,
                                                       const uint32_t *__restrict__ shift, uint64_t n_acc,
                                                       uint32_t *__restrict__ ok, uint32_t *__restrict__ bad) {
    __shared__ uint32_t l_st[kIlTxns + 1], l_sh[kIlTxns];
    __shared__ uint8_t l_own[kIlOwn];
    const uint32_t tiles = (s.tpr + kIlTxns - 1) / kIlTxns;
    const uint32_t q = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * kIlTxns;
    const uint32_t nj = s.tpr - j0 < kIlTxns ? s.tpr - j0 : kIlTxns;
    const uint64_t seg = s.eoff[q + 1] - s.eoff[q];
    for (uint32_t i = threadIdx.x; i <= nj; i += kBlock) l_st[i] = il_start(s, tbo, nullptr, q, j0 + i);
    for (uint32_t i = threadIdx.x; i < nj; i += kBlock) l_sh[i] = shift[(uint64_t)q * s.tpr + j0 + i];
    __syncthreads();
    const uint32_t a0 = l_st[0], a1 = l_st[nj];
    bool b = a1 < a0 || a1 > seg;
    const bool own = !b && a1 - a0 <= kIlOwn;
    if (own)
        for (uint32_t i = threadIdx.x; i < nj; i += kBlock)
            for (uint32_t a = l_st[i]; a < l_st[i + 1] && a >= a0 && a < a1; a++) l_own[a - a0] = (uint8_t)i;
    __syncthreads();
    for (uint32_t p = a0 + threadIdx.x; !b && p < a1; p += kBlock) {
        uint32_t lo = 0;
        if (own) {
            lo = l_own[p - a0];
        } else {
            uint32_t hi = nj;  // largest k with l_st[k] <= p
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (l_st[mid] <= p) lo = mid;
                else hi = mid;
            }
        }
        if (lo >= nj) {  // (boundaries a sender already reported bad)
            b = true;
            break;
        }
        // (k_il_begin checked the boundaries: the stores need only stay
        // inside the epoch when it found them bad)
        const uint64_t d = (uint64_t)p + l_sh[lo];
        if (d < n_acc) ok[d] = rk[s.eoff[q] + p];
        else b = true;
    }
    if (b) atomicOr(bad, 1u);
}

// the decided commit bytes back in origin order: out[q * tpr + j] = v[j * P + q]
__global__ __launch_bounds__(kBlock) void k_il_commits(const uint8_t *__restrict__ v, XSegs s,
                                                       uint8_t *__restrict__ out) {
    const uint64_t n = (uint64_t)s.P * s.tpr;
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kBlock) {
        uint64_t j = 0;
        const uint64_t q = divmod_magic(x, s.tpr, s.mT, j);
        out[x] = v[j * s.P + q];
    }
}

// ---- the list protocol in position-major order (DV_COMM_POSITION_ORDER; not
// CALVIN).  An owner receives, from every origin q, the records of q's txns
// that touch its rows, txn ids j * P + q rising inside q's segment; the
// partition's epoch wants them txn by txn in sequence order.  k_il_begin
// places txn j * P + q after txns 0..j of origins < q and 0..j-1 of origins
// >= q (from where each txn starts inside its segment: k_ilist_bounds), and
// k_ilist_move writes every record's fields to its place -- the split of the
// records (k_split_access) and the interleave in one pass.

// tbo[q * (tpr + 1) + j]: where txn j * P + q starts inside origin q's
// segment of the received records (a lower bound over the segment's ids)
__global__ __launch_bounds__(kBlock) void k_ilist_bounds(const dv_access *__restrict__ rec, XSegs s,
                                                         uint32_t *__restrict__ tbo, uint32_t *__restrict__ ncnt) {
    const uint64_t n = (uint64_t)s.P * (s.tpr + 1);
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kBlock) {
        const uint32_t q = (uint32_t)(x / (s.tpr + 1)), j = (uint32_t)(x % (s.tpr + 1));
        const uint64_t t = (uint64_t)j * s.P + q;  // (j == tpr: past every id of the segment)
        uint64_t lo = s.eoff[q], hi = s.eoff[q + 1];
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((uint64_t)rec[mid].txn_seq < t) lo = mid + 1;
            else hi = mid;
        }
        tbo[x] = (uint32_t)(lo - s.eoff[q]);
        if (j == 0) ncnt[q] = s.tpr + 1;
    }
}

// every received record to its place in sequence order: keys, types, txn
// ids, tables and (TPC-C) operation words.  A record whose id is past the
// epoch, not its origin's or out of order is not moved: ERRB_TXN in *err,
// which the epoch's error combine makes every rank's (k_refusal_err)
__global__ __launch_bounds__(kBlock) void k_ilist_move(const dv_access *__restrict__ rec,
                                                       const uint64_t *__restrict__ args, XSegs s,
                                                       const uint32_t *__restrict__ shift,
                                                       const uint32_t *__restrict__ tb, uint64_t n_acc,
                                                       uint64_t *__restrict__ keys, uint8_t *__restrict__ types,
                                                       uint32_t *__restrict__ txn, uint8_t *__restrict__ tables,
                                                       uint64_t *__restrict__ args_out, uint32_t *__restrict__ err) {
    const uint32_t n = s.P * s.tpr;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_acc; i += (uint64_t)gridDim.x * kBlock) {
        uint32_t q = 0;
        while (q + 1 < s.P && s.eoff[q + 1] <= i) q++;
        const dv_access a = rec[i];
        const uint32_t v = a.txn_seq;
        uint64_t qq = 0;
        const uint32_t j = (uint32_t)divmod_magic(v, s.P, s.mP, qq);
        bool good = v < n && (uint32_t)qq == q && (i == s.eoff[q] || rec[i - 1].txn_seq <= v);
        if (good) {
            const uint64_t d = (i - s.eoff[q]) + shift[(uint64_t)q * s.tpr + j];
            good = d < n_acc && d >= tb[v] && d < tb[v + 1];
            if (good) {
                keys[d] = a.key;
                types[d] = a.type;
                txn[d] = v;
                tables[d] = a.table;
                if (args_out) args_out[d] = args[i];
            }
        }
        bad |= !good;
    }
    if (bad) atomicOr(err, ERRB_TXN);
}

// per-txn values back in origin order: out[q * tpr + j] = v[j * P + q]
__global__ __launch_bounds__(kBlock) void k_il_words(const uint64_t *__restrict__ v, XSegs s,
                                                     uint64_t *__restrict__ out) {
    const uint64_t n = (uint64_t)s.P * s.tpr;
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kBlock) {
        uint64_t j = 0;
        const uint64_t q = divmod_magic(x, s.tpr, s.mT, j);
        out[x] = v[j * s.P + q];
    }
}

// the interleave's refusal as the epoch's only input error: the refused
// records left holes the probe reads as missing keys, but the batch is what
// is malformed (DV_ERR_TXN_RANGE, as a refused replicated epoch returns)
__global__ void k_refusal_err(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src) {
    if (threadIdx.x == 0 && *src) *dst = *src;
}

__global__ __launch_bounds__(kBlock) void k_rep_pack(const uint64_t *__restrict__ keys,
                                                     const uint8_t *__restrict__ types,
                                                     const uint32_t *__restrict__ txn, uint64_t n,
                                                     uint32_t tpr, uint32_t txn_base, uint32_t *__restrict__ k32,
                                                     uint32_t *__restrict__ t32, uint8_t *__restrict__ ty) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t k = keys[i];
        k32[i] = (k >> 32) ? 0xFFFFFFFFu : (uint32_t)k;
        t32[i] = global_txn(txn[i], tpr, txn_base);
        ty[i] = types[i];
    }
}


// ---- epoch groups (run_group): a group is P consecutive epochs; rank e
// decides epoch e of the group alone (the replicated single-GPU path over the
// epoch's batches, which every rank sends it), then routes the epoch's
// committed accesses to their owners, and every rank executes the records of
// epochs 0..P-1 on its rows, in epoch order.  Decisions depend only on an
// epoch's accesses, so deciding P epochs side by side gives
// the decisions of deciding them one after the other; execution keeps the
// epoch order on every row.

// lanes holding the same owner (restricted to `valid`); owners < 2^obits
__device__ __forceinline__ uint64_t match_owner(uint32_t o, uint64_t valid, uint32_t obits) {
    uint64_t peers = valid;
    for (uint32_t b = 0; b < obits; b++) {
        const uint32_t bit = (o >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// the committed txns' accesses, as k_exec_txn walks them (a wave takes 64
// txns and spreads their accesses over its lanes); emit(valid, global row,
// flags, txn) is called by every lane, wave-uniformly
template <class Emit>
__device__ __forceinline__ void walk_committed_txns(const uint32_t *__restrict__ tb_start,
                                                    const uint32_t *__restrict__ tb_end,
                                                    const uint32_t *__restrict__ acc_row, const RecRows &rr,
                                                    uint32_t n_txn, const uint8_t *__restrict__ status,
                                                    Emit &emit) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t step = gridDim.x * (kBlock / 64) * 64;
    for (uint32_t base = (blockIdx.x * (kBlock / 64) + wave) * 64; base < n_txn; base += step) {
        const uint32_t t = base + lane;
        const bool com = t < n_txn && status[t] == ST_COMMIT;
        if (__ballot(com) == 0) continue;
        const uint32_t a0 = com ? tb_start[t] : 0u;
        const uint32_t len = com ? tb_end[t] - a0 : 0u;
        uint32_t incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, 64);
            if (lane >= (uint32_t)off) incl += o;
        }
        const uint32_t pre = incl - len, total = __shfl(incl, 63, 64);
        for (uint32_t g0 = 0; g0 < total; g0 += 64) {
            const uint32_t g = g0 + lane;
            uint32_t src = 0;
#pragma unroll
            for (uint32_t w = 32; w > 0; w >>= 1) {
                const uint32_t cand = src + w;
                const uint32_t pv = __shfl(pre, (int)(cand & 63u), 64);
                if (cand < 64 && pv <= g) src = cand;
            }
            const uint32_t sa0 = __shfl(a0, (int)src, 64), spre = __shfl(pre, (int)src, 64);
            const bool v = g < total;
            const uint32_t ar = v ? row_word(acc_row, rr, sa0 + (g - spre)) : 0u;
            emit(v, ar & ~AR_WR, (ar & AR_WR) ? RT_WR : 0u, base + src);
        }
    }
}

// CALVIN: every committed access in row order (k_exec's view: a read after
// an earlier write of its queue sees that write)
template <class Emit>
__device__ __forceinline__ void walk_row_queues(const uint64_t *__restrict__ pairs, const uint64_t *__restrict__ el,
                                                const uint8_t *__restrict__ ew, uint64_t n,
                                                const uint8_t *__restrict__ status, Emit &emit) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t base = ((uint64_t)blockIdx.x * (kBlock / 64) + wave) * 64; base < n; base += step) {
        const uint64_t i = base + lane;
        const uint64_t e = i < n ? el[i] : 0ull;
        const bool v = i < n && status[el_txn(e)] == ST_COMMIT;
        const uint32_t wr = (e & EL_WR) ? RT_WR : 0u;
        const uint32_t seen = (v && !wr && ew && ew[i]) ? RT_SEESW : 0u;
        emit(v, v ? pair_row(pairs[i]) : 0u, wr | seen, el_txn(e));
    }
}

template <int SRC>
struct RouteSrc {
    const uint32_t *tb_start, *tb_end, *acc_row;
    uint32_t n_txn;
    const uint64_t *pairs, *el;
    const uint8_t *ew;
    uint64_t n;
    const uint8_t *status;
    RecRows rr;  // (SRC 0: the row words from the epoch's records instead of acc_row)
    template <class Emit>
    __device__ void walk(Emit &emit) const {
        if (SRC == 0) walk_committed_txns(tb_start, tb_end, acc_row, rr, n_txn, status, emit);
        else walk_row_queues(pairs, el, ew, n, status, emit);
    }
};

__host__ __device__ inline uint32_t owner_bits(uint32_t P) {
    uint32_t b = 0;
    while ((1u << b) < P) b++;
    return b;
}

// pass 1: records per owner per block (a halted or rejected epoch routes
// nothing: zero counts).  The txn walk (SRC 0) also writes the epoch's commit
// bytes (commit, may be null) and adds its committed count, as k_commit_out
// would one launch later
template <int SRC>
__global__ __launch_bounds__(kBlock) void k_route_count(RouteSrc<SRC> src, RouteOut ro, Counters *ctr,
                                                        uint8_t *__restrict__ commit) {
    __shared__ uint32_t c[kRadix];
    __shared__ uint32_t part[kBlock / 64];
    for (uint32_t o = threadIdx.x; o < ro.P; o += kBlock) c[o] = 0;
    if (SRC == 0 && !ctr->halt) {  // (halted: the rounds resume first, dv_epoch_finish)
        uint32_t cnt = commit_bytes_grid(src.status, src.n_txn, commit);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int w = 0; w < kBlock / 64; w++) t += part[w];
            if (t) atomicAdd(&my_slot(ctr).committed, t);
        }
    }
    __syncthreads();
    if (!(input_err(ctr) || ctr->halt)) {
        const uint32_t lane = threadIdx.x & 63, P = ro.P, ob = owner_bits(P);
        auto emit = [&](bool v, uint32_t row, uint32_t, uint32_t) {
            const uint32_t o = v ? row % P : 0u;
            const uint64_t peers = match_owner(o, __ballot(v), ob);
            if (v && lane == (uint32_t)__builtin_ctzll(peers)) atomicAdd(&c[o], (uint32_t)__popcll(peers));
        };
        src.walk(emit);
    }
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < ro.P; o += kBlock) ro.blk[o * kRouteBlocks + blockIdx.x] = c[o];
}

// this rank's outcome record, all-gathered (epoch groups, step 4): failure
// code, committed txns, receive capacity, refused, then records per owner
constexpr uint32_t kGroupRecHead = 8;

// per owner (one block each): the blocks' counts -> exclusive prefix in
// place, tot[o] = the owner's records; orec: the outcome record of a decided
// epoch group too (a failed decision's is written again by k_route_words)
__global__ __launch_bounds__(kBlock) void k_route_scan(RouteOut ro) {
    __shared__ uint32_t lds4[4];
    uint32_t *c = ro.blk + (uint64_t)blockIdx.x * kRouteBlocks;
    constexpr uint32_t per = kRouteBlocks / kBlock;
    uint32_t v[per], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        v[j] = c[threadIdx.x * per + j];
        sum += v[j];
    }
    uint32_t t = 0;
    uint32_t pre = block_excl_scan256(sum, lds4, &t);
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        c[threadIdx.x * per + j] = pre;
        pre += v[j];
    }
    if (threadIdx.x == 0) ro.tot[blockIdx.x] = t;
    if (ro.orec) {  // the outcome record, as k_route_words writes it for a decided epoch
        // (a refused batch decides the code; else the decision's error bits)
        const bool refused = *ro.bad != 0;
        const uint32_t fail = refused ? (uint32_t)(-DV_ERR_ARG) : (uint32_t)(-err_code_of(ro.ctr->err | ro.ctr->peer_err));
        if (threadIdx.x == 0) ro.orec[kGroupRecHead + blockIdx.x] = fail ? 0u : t;
        if (blockIdx.x == 0) {
            for (uint32_t i = threadIdx.x; i < 2u * kSlots; i += kBlock) ro.xacc[i] = 0;
            uint64_t committed = 0;  // (wave 0: a slot per lane, all loads in flight at once)
            for (uint32_t k = threadIdx.x; k < (uint32_t)kSlots && threadIdx.x < 64; k += 64)
                committed += ro.ctr->slot[k].committed;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) committed += __shfl_down(committed, off, 64);
            if (threadIdx.x == 0) {
                ro.orec[0] = fail;
                ro.orec[1] = fail ? 0u : committed;
                ro.orec[2] = ro.cap;
                ro.orec[3] = refused ? 1u : 0u;
                // a halted decision (its rounds yielded): its route was a
                // no-op; the decider finishes it and every rank votes again
                ro.orec[4] = !fail && (ro.ctr->halt | ro.ctr->a_halt) ? 1u : 0u;
                for (uint32_t k = 5; k < kGroupRecHead; k++) ro.orec[k] = 0;
            }
        }
    }
}

// pass 2: the same walk (same grid, same items per block), each block
// writing at its owner-major offsets
template <int SRC>
__global__ __launch_bounds__(kBlock) void k_route_scatter(RouteSrc<SRC> src, RouteOut ro, const Counters *ctr) {
    __shared__ uint32_t cur[kRadix];
    const uint32_t P = ro.P;
    if (input_err(ctr) || ctr->halt) return;
    for (uint32_t o = threadIdx.x; o < P; o += kBlock) {
        uint32_t off = 0;
        for (uint32_t q = 0; q < o; q++) off += ro.tot[q];
        cur[o] = off + ro.blk[o * kRouteBlocks + blockIdx.x];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, ob = owner_bits(P);
    auto emit = [&](bool v, uint32_t row, uint32_t flags, uint32_t txn) {
        const uint32_t o = v ? row % P : 0u;
        const uint64_t peers = match_owner(o, __ballot(v), ob);
        const uint32_t leader = v ? (uint32_t)__builtin_ctzll(peers) : lane;
        uint32_t b = 0;
        if (v && lane == leader) b = atomicAdd(&cur[o], (uint32_t)__popcll(peers));
        b = __shfl(b, (int)leader, 64);
        if (v) ro.rec[b + mask_rank(peers)] = make_uint2((row / P) | flags, txn);
    };
    src.walk(emit);
}

// run_ycsb_1 (ycsb_txn.cpp:227-254) of one epoch's routed records on this
// partition's rows: a read adds mix64(v ^ mix64(txn << 32 ^ pkey)) to the
// digest (v = 0 when it sees an earlier write of its epoch), a write stores 0
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_route_exec(const uint2 *__restrict__ rec, uint64_t n,
                                                       uint64_t *__restrict__ f0, const uint64_t *__restrict__ pkey,
                                                       unsigned long long *acc) {
    __shared__ unsigned long long part[2][4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long dig = 0, wcnt = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint2 r = rec[i];
        const uint32_t row = r.x & ~(RT_WR | RT_SEESW);
        if (r.x & RT_WR) {
            if (MODE & 2) {
                f0[row] = 0;  // *(uint64_t*)&data[0] = 0 (ycsb_txn.cpp:239-242)
                wcnt++;
            }
        } else if (MODE & 1) {
            const uint64_t val = (r.x & RT_SEESW) ? 0ull : f0[row];
            dig += mix64(val ^ mix64(((uint64_t)r.y << 32) ^ pkey[row]));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        dig += __shfl_down(dig, off, 64);
        wcnt += __shfl_down(wcnt, off, 64);
    }
    if (lane == 0) {
        part[0][wave] = dig;
        part[1][wave] = wcnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long d = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const unsigned long long w = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        // line-separated slots: one word takes ~88 device-scope adds per us
        if (d) atomicAdd(&acc[2 * (blockIdx.x & (kSlots - 1))], d);
        if (w) atomicAdd(&acc[2 * (blockIdx.x & (kSlots - 1)) + 1], w);
    }
}

// ---- host round trips without blits or stream synchronisation: small
// host values reach the device as kernel arguments (k_put_words), device
// values reach the host through a host-mapped mailbox written by one kernel
// with system-scope stores and a sequence word the host spins on
struct PutArgs {
    uint64_t v64[kRadix + 8];
    uint32_t v32[8];
    uint32_t n64, n32;
    uint64_t *d64;
    uint32_t *d32;
};
__global__ void k_put_words(PutArgs a) {
    for (uint32_t i = threadIdx.x; i < a.n64; i += blockDim.x) a.d64[i] = a.v64[i];
    for (uint32_t i = threadIdx.x; i < a.n32; i += blockDim.x) a.d32[i] = a.v32[i];
}

struct CommMail {
    unsigned long long seq;
    unsigned long long pad[7];
    unsigned long long w[1];  // (allocated for mail_words(P) words)
};
__host__ __device__ inline uint64_t mail_words(uint32_t P) { return 4ull * kRadix + (uint64_t)P * (8 + P); }
__global__ void k_mail_out(const uint64_t *__restrict__ a, uint32_t na, const uint32_t *__restrict__ b, uint32_t nb,
                           const uint64_t *__restrict__ c, uint32_t nc, CommMail *m, unsigned long long seq) {
    for (uint32_t i = threadIdx.x; i < na; i += blockDim.x) m->w[i] = a[i];
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) m->w[na + i] = b[i];
    for (uint32_t i = threadIdx.x; i < nc; i += blockDim.x) m->w[na + nb + i] = c[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&m->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// (this rank's outcome record: kGroupRecHead, k_route_words)
// (and the execution's digest slots zeroed for step 6: the previous group's
// were read by this group's vote)
__global__ void k_route_words(const uint32_t *__restrict__ tot, uint32_t P, uint64_t committed, uint32_t fail,
                              uint64_t cap, uint64_t *__restrict__ rec, uint32_t *__restrict__ pack_bad,
                              unsigned long long *__restrict__ xacc) {
    for (uint32_t i = threadIdx.x; i < 2u * kSlots; i += blockDim.x) xacc[i] = 0;
    // a compact batch with txn ids that are not dense (k_group_pack_c), or a
    // batch the position-major move refused (k_il_move), fails the group as an
    // argument error -- whatever its decision made of the input; the flag is
    // reset for the next group
    const bool refused = *pack_bad != 0;
    if (refused) fail = (uint32_t)(-DV_ERR_ARG);
    __syncthreads();
    if (threadIdx.x == 0) *pack_bad = 0;
    for (uint32_t q = threadIdx.x; q < P; q += blockDim.x) rec[kGroupRecHead + q] = fail ? 0u : tot[q];
    if (threadIdx.x == 0) {
        rec[0] = fail;
        rec[1] = committed;
        rec[2] = cap;
        rec[3] = refused ? 1u : 0u;  // (a refused batch decides the group's code on every rank)
        for (uint32_t k = 4; k < kGroupRecHead; k++) rec[k] = 0;
    }
}

void launch_route_txn(hipStream_t s, const RouteOut &ro, const uint32_t *tb_start, const uint32_t *tb_end,
                      const uint32_t *acc_row, const RecRows &rr, uint32_t n_txn, const uint8_t *status,
                      Counters *ctr, uint8_t *d_commit) {
    const RouteSrc<0> src{tb_start, tb_end, acc_row, n_txn, nullptr, nullptr, nullptr, 0, status, rr};
    DV_LAUNCH((k_route_count<0>), kRouteBlocks, kBlock, 0, s, src, ro, ctr, d_commit);
    DV_LAUNCH(k_route_scan, ro.P, kBlock, 0, s, ro);
    if (ro.wrote) *ro.wrote = ro.orec != nullptr;
    DV_LAUNCH((k_route_scatter<0>), kRouteBlocks, kBlock, 0, s, src, ro, ctr);
}

void launch_route_rowq(hipStream_t s, const RouteOut &ro, const uint64_t *pairs, const uint64_t *el,
                       const uint8_t *ew, uint64_t n, const uint8_t *status, Counters *ctr) {
    const RouteSrc<1> src{nullptr, nullptr, nullptr, 0, pairs, el, ew, n, status, RecRows{}};
    DV_LAUNCH((k_route_count<1>), kRouteBlocks, kBlock, 0, s, src, ro, ctr, (uint8_t *)nullptr);
    RouteOut r0 = ro;  // (CALVIN's commit count comes after the route: k_route_words writes the record)
    r0.orec = nullptr;
    DV_LAUNCH(k_route_scan, ro.P, kBlock, 0, s, r0);
    DV_LAUNCH((k_route_scatter<1>), kRouteBlocks, kBlock, 0, s, src, ro, ctr);
}

// ---- in-process group: element-wise MAX of the P ranks' buffers
constexpr int kMaxLocalRanks = 16;
template <class T>
struct PeerPtrs {
    const T *p[kMaxLocalRanks];
};
template <class T>
__global__ __launch_bounds__(kBlock) void k_max_reduce(PeerPtrs<T> in, int P, T *__restrict__ out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        T v = in.p[0][i];
        for (int q = 1; q < P; q++) v = in.p[q][i] > v ? in.p[q][i] : v;
        out[i] = v;
    }
}

struct Xport;  // the collectives of one rank (below)

struct DvComm {
    Xport *x = nullptr;
    int nranks = 0, rank = 0;
    uint64_t acc_cap = 0;  // capacity of the record / SoA buffers
    uint32_t nb_cap = 0, txn_cap = 0;
    dv_access *send = nullptr, *recv = nullptr;
    uint64_t *send_args = nullptr, *recv_args = nullptr;  // TPC-C operation words, routed like the records
    uint64_t *keys = nullptr;
    uint8_t *types = nullptr, *tables = nullptr, *verdict = nullptr;
    uint32_t *txn = nullptr, *counts = nullptr, *tot = nullptr, *err = nullptr;
    uint64_t *xcnt = nullptr;  // [2 * nranks]: send counts, received counts
    uint32_t *xvote = nullptr; // [8]: longest txn, argument flags, longest batch, replication blockers (MAX); groups: table widths
    int mode = 0;              // dv_comm_set_mode: 0 automatic, 1 list protocol, 2 replicated when possible
    bool wide = false;         // epoch groups: 8-byte batches even where the compact ones fit (DV_COMM_WIDE_BATCHES)
    uint32_t *gerr = nullptr;  // input-error bits, all-reduced (MAX)
    CommMail *h_mail = nullptr, *d_mail = nullptr;  // host-mapped mailbox (mail_wait)
    unsigned long long mseq = 0;
    // epoch groups (run_group)
    uint32_t *rblk = nullptr, *rtot = nullptr;  // route counts: [P][kRouteBlocks], [P]
    uint8_t *gcommit = nullptr;                 // the commit bytes when the caller passes none
    unsigned long long *xacc = nullptr;         // execution: read digest, writes ([2][kSlots])
    uint64_t *gs = nullptr, *gr = nullptr;      // all-gathered vote / outcome records: [8 + P], [P][8 + P]
    uint32_t *gtc = nullptr;                    // compact batches: txn starts per received tile
    uint32_t *gbad = nullptr;                   // compact batches: a sender's txn ids were not dense
    bool position = false;                      // epoch groups: position-major (DV_COMM_POSITION_ORDER)
    uint32_t *ilk = nullptr, *ilt = nullptr;    // position-major: the interleaved epoch's rows, txn ids
    uint32_t *tbo = nullptr, *ncnt = nullptr;   // k_il_begin's inputs
    uint32_t *iltb = nullptr, *ilsh = nullptr;  // ... its outputs: the decider's txn_begin, the move's shifts
    uint8_t *ilv = nullptr;                     // commit bytes back in origin order
    uint64_t *iloid = nullptr;                  // TPC-C list protocol, position-major: o_id by sequence number
    uint32_t *tbr = nullptr;                    // tbx: the batches' txn_begin as landed (tpr + 1 words each)
};

}  // namespace dvcc

using namespace dvcc;

namespace {

int nccl_fail(ncclResult_t e, const char *what) {
    if (e == ncclSuccess) return DV_OK;
    std::fprintf(stderr, "dvcc: %s failed: %s\n", what, ncclGetErrorString(e));
    return DV_ERR_HIP;
}
int hip_fail2(hipError_t e, const char *what) {
    if (e == hipSuccess) return DV_OK;
    std::fprintf(stderr, "dvcc: %s failed: %s\n", what, hipGetErrorString(e));
    return DV_ERR_HIP;
}
#define CHK(x)                 \
    do {                       \
        int _r = (x);          \
        if (_r) return _r;     \
    } while (0)

template <class T>
int alloc(T **p, uint64_t n) {
    return hip_fail2(hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * (n ? n : 1)), "hipMalloc");
}

}  // namespace

// The four collectives of the partitioned epoch, issued on the context's
// stream in the same order by every rank.  RCCL between processes (one per
// GPU, over xGMI) is the product; the in-process group runs the same driver
// for P contexts in one process -- several partitions on one GPU -- so the
// multi-rank protocol is tested on a one-GPU box.
struct dvcc::Xport {
    virtual ~Xport() = default;
    // one u64 to every peer, one from every peer
    virtual int all_to_all_u64(const uint64_t *send, uint64_t *recv, hipStream_t s) = 0;
    // collectives issued between group(true) and group(false) may progress
    // together (RCCL: ncclGroupStart / ncclGroupEnd)
    virtual int group(bool begin) {
        (void)begin;
        return DV_OK;
    }
    // bytes: send segment [sd[q], sd[q] + sc[q]) to peer q, receive rc[q] at rd[q]
    virtual int all_to_allv(const uint8_t *send, const size_t *sc, const size_t *sd, uint8_t *recv,
                            const size_t *rc, const size_t *rd, hipStream_t s) = 0;
    // the same with a buffer of its own per peer: send[q] (sc[q] bytes) to peer q
    virtual int all_to_allv_segs(const uint8_t *const *send, const size_t *sc, uint8_t *recv, const size_t *rc,
                                 const size_t *rd, hipStream_t s) = 0;
    // in place, element-wise MAX
    virtual int max_u32(uint32_t *buf, uint64_t n, hipStream_t s) = 0;
    virtual int max_u8(uint8_t *buf, uint64_t n, hipStream_t s) = 0;
    virtual int max_u64(uint64_t *buf, uint64_t n, hipStream_t s) = 0;
    // `bytes` from every rank, rank q's at recv + q * bytes
    virtual int all_gather(const uint8_t *send, size_t bytes, uint8_t *recv, hipStream_t s) = 0;
};

namespace {

struct RcclXport final : Xport {
    ncclComm_t comm = nullptr;
    int P = 0;
    ~RcclXport() override {
        if (comm) (void)ncclCommDestroy(comm);
    }
    int group(bool begin) override {
        return nccl_fail(begin ? ncclGroupStart() : ncclGroupEnd(), begin ? "ncclGroupStart" : "ncclGroupEnd");
    }
    int all_to_all_u64(const uint64_t *send, uint64_t *recv, hipStream_t s) override {
        return nccl_fail(ncclAllToAll(send, recv, 1, ncclUint64, comm, s), "ncclAllToAll");
    }
    int all_to_allv(const uint8_t *send, const size_t *sc, const size_t *sd, uint8_t *recv, const size_t *rc,
                    const size_t *rd, hipStream_t s) override {
        return nccl_fail(ncclAllToAllv(send, sc, sd, recv, rc, rd, ncclUint8, comm, s), "ncclAllToAllv");
    }
    int all_to_allv_segs(const uint8_t *const *send, const size_t *sc, uint8_t *recv, const size_t *rc,
                         const size_t *rd, hipStream_t s) override {
        int r = nccl_fail(ncclGroupStart(), "ncclGroupStart");
        for (int q = 0; q < P && !r; q++) {
            if (sc[q]) r = nccl_fail(ncclSend(send[q], sc[q], ncclUint8, q, comm, s), "ncclSend");
            if (!r && rc[q]) r = nccl_fail(ncclRecv(recv + rd[q], rc[q], ncclUint8, q, comm, s), "ncclRecv");
        }
        const int e = nccl_fail(ncclGroupEnd(), "ncclGroupEnd");
        return r ? r : e;
    }
    int max_u32(uint32_t *buf, uint64_t n, hipStream_t s) override {
        return nccl_fail(ncclAllReduce(buf, buf, n, ncclUint32, ncclMax, comm, s), "ncclAllReduce");
    }
    int max_u8(uint8_t *buf, uint64_t n, hipStream_t s) override {
        return nccl_fail(ncclAllReduce(buf, buf, n, ncclUint8, ncclMax, comm, s), "ncclAllReduce");
    }
    int max_u64(uint64_t *buf, uint64_t n, hipStream_t s) override {
        return nccl_fail(ncclAllReduce(buf, buf, n, ncclUint64, ncclMax, comm, s), "ncclAllReduce");
    }
    int all_gather(const uint8_t *send, size_t bytes, uint8_t *recv, hipStream_t s) override {
        return nccl_fail(ncclAllGather(send, recv, bytes, ncclUint8, comm, s), "ncclAllGather");
    }
};

// P ranks in one process, each driven by its own host thread.  A collective:
// every rank publishes its buffers and an event behind the data on its
// stream; host barrier; every rank makes its stream wait for the peers'
// events and pulls (device copies, or a MAX kernel into private scratch);
// it records a second event; host barrier; every rank waits for all
// second events -- no peer still reads its buffers -- before it writes the
// result in place or goes on.
struct LocalGroup {
    int P = 0;
    int refs = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    struct Slot {
        const uint8_t *send = nullptr;
        const size_t *sd = nullptr;
        const uint8_t *const *segs = nullptr;  // all_to_allv_segs: the buffer per peer
        hipEvent_t ready = nullptr, done = nullptr;
    };
    std::vector<Slot> slot;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t g = gen;
        if (++arrived == P) {
            arrived = 0;
            gen++;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
    }
};

struct LocalXport final : Xport {
    LocalGroup *g = nullptr;
    int r = 0;
    uint8_t *scratch = nullptr;  // all-reduce result before it goes in place
    uint64_t scratch_cap = 0;
    ~LocalXport() override {
        if (scratch) (void)hipFree(scratch);
        LocalGroup::Slot &me = g->slot[r];
        if (me.ready) (void)hipEventDestroy(me.ready);
        if (me.done) (void)hipEventDestroy(me.done);
        bool last = false;
        {
            std::lock_guard<std::mutex> lk(g->mu);
            last = --g->refs == 0;
        }
        if (last) delete g;
    }
    int publish(const uint8_t *send, const size_t *sd, hipStream_t s) {
        g->slot[r].send = send;
        g->slot[r].sd = sd;
        CHK(hip_fail2(hipEventRecord(g->slot[r].ready, s), "hipEventRecord"));
        g->barrier();
        for (int q = 0; q < g->P; q++) CHK(hip_fail2(hipStreamWaitEvent(s, g->slot[q].ready, 0), "wait"));
        return DV_OK;
    }
    int retire(hipStream_t s) {
        CHK(hip_fail2(hipEventRecord(g->slot[r].done, s), "hipEventRecord"));
        g->barrier();
        for (int q = 0; q < g->P; q++) CHK(hip_fail2(hipStreamWaitEvent(s, g->slot[q].done, 0), "wait"));
        g->barrier();  // every rank has queued its waits before any event is recorded again
        return DV_OK;
    }
    int all_to_all_u64(const uint64_t *send, uint64_t *recv, hipStream_t s) override {
        CHK(publish(reinterpret_cast<const uint8_t *>(send), nullptr, s));
        for (int q = 0; q < g->P; q++)
            CHK(hip_fail2(hipMemcpyAsync(recv + q, reinterpret_cast<const uint64_t *>(g->slot[q].send) + r, 8,
                                         hipMemcpyDeviceToDevice, s), "copy"));
        return retire(s);
    }
    // all_to_allv and all_to_allv_segs are one collective: every sender picks
    // its own form (run_group's `direct` is a rank's own decision), as ncclSend
    // pairs with ncclAllToAllv over RCCL, so a peer's part for this rank is
    // read from whichever form it published
    const uint8_t *from(int q) const {
        const LocalGroup::Slot &p = g->slot[q];
        return p.segs ? p.segs[r] : p.send + p.sd[r];
    }
    int all_to_allv(const uint8_t *send, const size_t *sc, const size_t *sd, uint8_t *recv, const size_t *rc,
                    const size_t *rd, hipStream_t s) override {
        (void)sc;
        g->slot[r].segs = nullptr;
        CHK(publish(send, sd, s));
        for (int q = 0; q < g->P; q++)
            if (rc[q]) CHK(hip_fail2(hipMemcpyAsync(recv + rd[q], from(q), rc[q], hipMemcpyDeviceToDevice, s), "copy"));
        return retire(s);
    }
    int all_to_allv_segs(const uint8_t *const *send, const size_t *sc, uint8_t *recv, const size_t *rc,
                         const size_t *rd, hipStream_t s) override {
        (void)sc;
        g->slot[r].segs = send;  // (read by the peers after publish's barrier)
        CHK(publish(nullptr, nullptr, s));
        for (int q = 0; q < g->P; q++)
            if (rc[q]) CHK(hip_fail2(hipMemcpyAsync(recv + rd[q], from(q), rc[q], hipMemcpyDeviceToDevice, s), "copy"));
        return retire(s);
    }
    template <class T>
    int max_t(T *buf, uint64_t n, hipStream_t s) {
        if (n * sizeof(T) > scratch_cap) {
            CHK(hip_fail2(hipStreamSynchronize(s), "sync"));
            if (scratch) (void)hipFree(scratch);
            scratch = nullptr;
            scratch_cap = 0;
            CHK(alloc(&scratch, n * sizeof(T)));
            scratch_cap = n * sizeof(T);
        }
        CHK(publish(reinterpret_cast<const uint8_t *>(buf), nullptr, s));
        PeerPtrs<T> in{};
        for (int q = 0; q < g->P; q++) in.p[q] = reinterpret_cast<const T *>(g->slot[q].send);
        if (n) {
            const uint64_t blocks = std::min<uint64_t>((n + kBlock - 1) / kBlock, 2048);
            DV_LAUNCH((k_max_reduce<T>), (uint32_t)blocks, kBlock, 0, s, in, g->P, reinterpret_cast<T *>(scratch), n);
            CHK(hip_fail2(hipGetLastError(), "k_max_reduce"));
        }
        CHK(retire(s));
        if (n) CHK(hip_fail2(hipMemcpyAsync(buf, scratch, n * sizeof(T), hipMemcpyDeviceToDevice, s), "copy"));
        return DV_OK;
    }
    int max_u32(uint32_t *buf, uint64_t n, hipStream_t s) override { return max_t(buf, n, s); }
    int max_u8(uint8_t *buf, uint64_t n, hipStream_t s) override { return max_t(buf, n, s); }
    int max_u64(uint64_t *buf, uint64_t n, hipStream_t s) override { return max_t(buf, n, s); }
    int all_gather(const uint8_t *send, size_t bytes, uint8_t *recv, hipStream_t s) override {
        CHK(publish(send, nullptr, s));
        for (int q = 0; q < g->P; q++)
            if (bytes)
                CHK(hip_fail2(hipMemcpyAsync(recv + (size_t)q * bytes, g->slot[q].send, bytes,
                                             hipMemcpyDeviceToDevice, s), "copy"));
        return retire(s);
    }
};

// P processes of one node (e.g. several ranks on one GPU, which RCCL
// refuses: ncclCommInitRank "invalid usage"), for testing the protocols across
// real process boundaries.  Each rank exports one device staging buffer
// through a HIP IPC handle and publishes it, with its all-to-allv offsets,
// in a POSIX shared-memory segment that also holds a process-shared barrier.
// A collective: the rank copies its payload into its staging buffer and
// drains its stream; barrier; it pulls from the peers' staging buffers
// (device copies, or a MAX kernel over them) and drains again; barrier -- so
// no peer still reads a staging buffer when it is written next.  Host-
// synchronous by design: test infrastructure, the product's transport is RCCL.
constexpr int kMaxIpcRanks = kMaxLocalRanks;
struct IpcShm {
    std::atomic<uint32_t> arrived, gen, joined;
    uint32_t P;
    struct Slot {
        hipIpcMemHandle_t h;
        uint64_t sd[kMaxIpcRanks];  // this rank's all-to-allv send offsets
        uint64_t staging_bytes;
        int32_t device;
    } slot[kMaxIpcRanks];
};
static_assert(std::atomic<uint32_t>::is_always_lock_free, "process-shared atomics");

struct IpcXport final : Xport {
    IpcShm *shm = nullptr;
    int P = 0, r = 0;
    uint8_t *staging = nullptr;  // this rank's, exported
    uint64_t staging_cap = 0;
    uint8_t *peer[kMaxIpcRanks] = {};  // every rank's staging buffer (own included)
    uint8_t *scratch = nullptr;
    uint64_t scratch_cap = 0;
    ~IpcXport() override {
        for (int q = 0; q < P; q++)
            if (q != r && peer[q]) (void)hipIpcCloseMemHandle(peer[q]);
        if (staging) (void)hipFree(staging);
        if (scratch) (void)hipFree(scratch);
        if (shm) (void)munmap(shm, sizeof(IpcShm));
    }
    // every rank arrives; a rank that does not come within 120 s (it died or
    // left the protocol) fails the others instead of hanging them
    int barrier() {
        const uint32_t g = shm->gen.load(std::memory_order_acquire);
        if (shm->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)P) {
            shm->arrived.store(0, std::memory_order_relaxed);
            shm->gen.fetch_add(1, std::memory_order_acq_rel);
            return DV_OK;
        }
        const auto t0 = std::chrono::steady_clock::now();
        while (shm->gen.load(std::memory_order_acquire) == g) {
            std::this_thread::yield();
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) return DV_ERR_STATE;
        }
        return DV_OK;
    }
    int stage(const uint8_t *src, uint64_t bytes, hipStream_t s) {
        if (bytes > staging_cap) return DV_ERR_ARG;
        if (bytes) CHK(hip_fail2(hipMemcpyAsync(staging, src, bytes, hipMemcpyDeviceToDevice, s), "stage"));
        CHK(hip_fail2(hipStreamSynchronize(s), "sync"));
        return barrier();
    }
    int drain(hipStream_t s) {
        CHK(hip_fail2(hipStreamSynchronize(s), "sync"));
        return barrier();
    }
    int all_to_all_u64(const uint64_t *send, uint64_t *recv, hipStream_t s) override {
        CHK(stage(reinterpret_cast<const uint8_t *>(send), 8ull * P, s));
        for (int q = 0; q < P; q++)
            CHK(hip_fail2(hipMemcpyAsync(recv + q, peer[q] + 8ull * r, 8, hipMemcpyDeviceToDevice, s), "copy"));
        return drain(s);
    }
    int all_to_allv(const uint8_t *send, const size_t *sc, const size_t *sd, uint8_t *recv, const size_t *rc,
                    const size_t *rd, hipStream_t s) override {
        uint64_t end = 0;
        for (int q = 0; q < P; q++) {
            shm->slot[r].sd[q] = sd[q];
            end = std::max<uint64_t>(end, sd[q] + sc[q]);
        }
        CHK(stage(send, end, s));
        for (int q = 0; q < P; q++)
            if (rc[q])
                CHK(hip_fail2(hipMemcpyAsync(recv + rd[q], peer[q] + shm->slot[q].sd[r], rc[q],
                                             hipMemcpyDeviceToDevice, s), "copy"));
        return drain(s);
    }
    int all_to_allv_segs(const uint8_t *const *send, const size_t *sc, uint8_t *recv, const size_t *rc,
                         const size_t *rd, hipStream_t s) override {
        uint64_t off = 0;
        for (int q = 0; q < P; q++) off += sc[q];
        if (off > staging_cap) return DV_ERR_ARG;
        off = 0;
        for (int q = 0; q < P; q++) {  // (the segments staged back to back)
            shm->slot[r].sd[q] = off;
            if (sc[q])
                CHK(hip_fail2(hipMemcpyAsync(staging + off, send[q], sc[q], hipMemcpyDeviceToDevice, s), "stage"));
            off += sc[q];
        }
        CHK(stage(nullptr, 0, s));
        for (int q = 0; q < P; q++)
            if (rc[q])
                CHK(hip_fail2(hipMemcpyAsync(recv + rd[q], peer[q] + shm->slot[q].sd[r], rc[q],
                                             hipMemcpyDeviceToDevice, s), "copy"));
        return drain(s);
    }
    template <class T>
    int max_t(T *buf, uint64_t n, hipStream_t s) {
        if (n * sizeof(T) > scratch_cap) {
            CHK(hip_fail2(hipStreamSynchronize(s), "sync"));
            if (scratch) (void)hipFree(scratch);
            scratch = nullptr;
            scratch_cap = 0;
            CHK(alloc(&scratch, n * sizeof(T)));
            scratch_cap = n * sizeof(T);
        }
        CHK(stage(reinterpret_cast<const uint8_t *>(buf), n * sizeof(T), s));
        PeerPtrs<T> in{};
        for (int q = 0; q < P; q++) in.p[q] = reinterpret_cast<const T *>(peer[q]);
        if (n) {
            const uint64_t blocks = std::min<uint64_t>((n + kBlock - 1) / kBlock, 2048);
            DV_LAUNCH((k_max_reduce<T>), (uint32_t)blocks, kBlock, 0, s, in, P, reinterpret_cast<T *>(scratch), n);
            CHK(hip_fail2(hipGetLastError(), "k_max_reduce"));
        }
        CHK(drain(s));
        if (n) CHK(hip_fail2(hipMemcpyAsync(buf, scratch, n * sizeof(T), hipMemcpyDeviceToDevice, s), "copy"));
        return DV_OK;
    }
    int max_u32(uint32_t *buf, uint64_t n, hipStream_t s) override { return max_t(buf, n, s); }
    int max_u8(uint8_t *buf, uint64_t n, hipStream_t s) override { return max_t(buf, n, s); }
    int max_u64(uint64_t *buf, uint64_t n, hipStream_t s) override { return max_t(buf, n, s); }
    int all_gather(const uint8_t *send, size_t bytes, uint8_t *recv, hipStream_t s) override {
        CHK(stage(send, bytes, s));
        for (int q = 0; q < P; q++)
            if (bytes)
                CHK(hip_fail2(hipMemcpyAsync(recv + (size_t)q * bytes, peer[q], bytes, hipMemcpyDeviceToDevice, s),
                              "copy"));
        return drain(s);
    }
};

// the largest payload one collective of a context's protocols stages
uint64_t ipc_staging_bytes(const dv_config &cfg, uint32_t P) {
    const uint64_t acc = cfg.max_acc, txn = cfg.max_txn;
    uint64_t b = std::max<uint64_t>(acc * sizeof(dv_access), 8 * txn);  // records; o_ids (TPC-C)
    b = std::max<uint64_t>(b, 8ull * (kGroupRecHead + P) + 64);          // vote records
    return (b + 255) & ~255ull;
}

void free_bufs(DvComm *m) {
    if (m->h_mail) (void)hipHostFree(m->h_mail);
    m->h_mail = m->d_mail = nullptr;
    void *b[] = {m->send, m->recv, m->send_args, m->recv_args, m->keys, m->types, m->tables, m->verdict, m->txn,
                 m->counts, m->tot, m->err, m->xcnt, m->xvote, m->gerr, m->rblk, m->rtot, m->gcommit, m->xacc,
                 m->gs, m->gr, m->gtc, m->gbad, m->ilk, m->ilt, m->tbo, m->ncnt, m->iltb, m->ilsh, m->ilv, m->tbr,
                 m->iloid};
    for (void *p : b)
        if (p) (void)hipFree(p);
    m->send = m->recv = nullptr;
    m->send_args = m->recv_args = nullptr;
    m->keys = nullptr;
    m->types = m->tables = m->verdict = nullptr;
    m->txn = m->counts = m->tot = m->err = m->xvote = m->gerr = nullptr;
    m->xcnt = nullptr;
    m->rblk = m->rtot = nullptr;
    m->gcommit = nullptr;
    m->xacc = nullptr;
    m->gs = m->gr = nullptr;
    m->gtc = m->gbad = nullptr;
    m->ilk = m->ilt = m->tbo = m->ncnt = m->iltb = m->ilsh = nullptr;
    m->ilv = nullptr;
    m->iloid = nullptr;
    m->tbr = nullptr;
}

// every buffer an epoch of this context can need, sized once (dv_comm_init):
// an allocation that fails inside an epoch would leave one rank outside the
// collectives the others enter
int reserve(DvComm *m, uint64_t acc, uint32_t txn, bool tpcc) {
    const uint32_t nb = nblocks_for(acc ? acc : 1);
    const uint32_t P = (uint32_t)m->nranks;
    CHK(alloc(&m->send, acc));
    CHK(alloc(&m->recv, acc));
    if (tpcc) {
        CHK(alloc(&m->send_args, acc));
        CHK(alloc(&m->recv_args, acc));
    }
    CHK(alloc(&m->keys, acc));
    CHK(alloc(&m->types, acc));
    CHK(alloc(&m->tables, acc));
    CHK(alloc(&m->txn, acc));
    CHK(alloc(&m->verdict, ((uint64_t)txn + 3) & ~3ull));
    CHK(alloc(&m->counts, (uint64_t)P * nb));
    CHK(alloc(&m->tot, P));
    CHK(alloc(&m->err, 1));
    CHK(alloc(&m->xcnt, 2ull * P));
    CHK(alloc(&m->xvote, 8));
    CHK(alloc(&m->gerr, 1));
    CHK(alloc(&m->rblk, (uint64_t)P * kRouteBlocks));
    CHK(alloc(&m->rtot, P));
    CHK(alloc(&m->gcommit, txn));
    CHK(alloc(&m->xacc, 2 * kSlots));
    CHK(alloc(&m->gs, kGroupRecHead + P));
    CHK(alloc(&m->gr, (uint64_t)P * (kGroupRecHead + P)));
    CHK(alloc(&m->gtc, acc / kXTile + kXMaxP + 2));
    CHK(alloc(&m->gbad, 1));
    CHK(hip_fail2(hipMemset(m->gbad, 0, sizeof(uint32_t)), "memset"));
    // the interleave's index arrays (position-major epoch groups, replicated
    // epochs and list-protocol epochs)
    CHK(alloc(&m->tbo, (uint64_t)txn + P));
    CHK(alloc(&m->ncnt, kXMaxP));
    CHK(alloc(&m->iltb, (uint64_t)txn + 1));
    CHK(alloc(&m->ilsh, txn));
    if (!tpcc) {  // (position-major epoch groups)
        CHK(alloc(&m->ilk, acc));
        CHK(alloc(&m->ilt, acc));
        CHK(alloc(&m->ilv, txn));
        CHK(alloc(&m->tbr, (uint64_t)txn + P));
    } else {
        CHK(alloc(&m->iloid, txn));
    }
    const size_t mail_bytes = sizeof(CommMail) + 8 * mail_words(P);
    CHK(hip_fail2(hipHostMalloc(reinterpret_cast<void **>(&m->h_mail), mail_bytes,
                                hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc"));
    CHK(hip_fail2(hipHostGetDevicePointer(reinterpret_cast<void **>(&m->d_mail), m->h_mail, 0),
                  "hipHostGetDevicePointer"));
    std::memset(m->h_mail, 0, mail_bytes);
    m->acc_cap = acc;
    m->nb_cap = nb;
    m->txn_cap = txn;
    return DV_OK;
}

}  // namespace

// replicated epochs: the probe's input-error bits combined over the ranks
// (MAX) into peer_err, on the stream -- a key missing on its owner rejects the
// epoch on every rank before anything executes
int comm_combine_errors(dv_ctx *c) {
    DvComm *m = ctx_comm(c);
    if (!m) return DV_ERR_STATE;
    hipStream_t s = ctx_stream(c);
    uint32_t *w = ctx_err_words(c);  // err, peer_err
    CHK(hip_fail2(hipMemcpyAsync(m->gerr, w, sizeof(uint32_t), hipMemcpyDeviceToDevice, s), "copy"));
    CHK(m->x->max_u32(m->gerr, 1, s));
    return hip_fail2(hipMemcpyAsync(w + 1, m->gerr, sizeof(uint32_t), hipMemcpyDeviceToDevice, s), "copy");
}

void comm_free(DvComm *m) {
    if (!m) return;
    free_bufs(m);
    delete m->x;
    delete m;
}

extern "C" {

int dv_comm_unique_id(void *id_out) {
    if (!id_out) return DV_ERR_ARG;
    ncclUniqueId id;
    CHK(nccl_fail(ncclGetUniqueId(&id), "ncclGetUniqueId"));
    std::memcpy(id_out, &id, sizeof(id));
    return DV_OK;
}

int dv_comm_init(dv_ctx *c, const void *unique_id, int nranks, int rank) {
    if (!c || !unique_id || nranks < 1 || nranks > kRadix || rank < 0 || rank >= nranks) return DV_ERR_ARG;
    const dv_config &cfg = ctx_config(c);
    if ((int)cfg.part_cnt != nranks || (int)cfg.part_id != rank) return DV_ERR_ARG;  // partition == rank
    CHK(hip_fail2(hipSetDevice(cfg.device), "hipSetDevice"));
    DvComm *&slot = ctx_comm(c);
    comm_free(slot);
    slot = new DvComm();
    slot->nranks = nranks;
    slot->rank = rank;
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    RcclXport *x = new RcclXport();
    x->P = nranks;
    slot->x = x;
    int r = nccl_fail(ncclCommInitRank(&x->comm, nranks, id, rank), "ncclCommInitRank");
    if (r) x->comm = nullptr;
    if (!r) r = reserve(slot, cfg.max_acc, cfg.max_txn, cfg.workload == DV_TPCC);
    if (r) {
        comm_free(slot);
        slot = nullptr;
    }
    return r;
}

int dv_comm_init_ipc(dv_ctx *c, const char *name, int nranks, int rank) {
    if (!c || !name || name[0] != '/' || nranks < 1 || nranks > kMaxIpcRanks || rank < 0 || rank >= nranks)
        return DV_ERR_ARG;
    const dv_config &cfg = ctx_config(c);
    if ((int)cfg.part_cnt != nranks || (int)cfg.part_id != rank) return DV_ERR_ARG;
    CHK(hip_fail2(hipSetDevice(cfg.device), "hipSetDevice"));
    DvComm *&slot = ctx_comm(c);
    comm_free(slot);
    slot = nullptr;
    // the segment: created by whoever comes first, sized once
    const int fd = shm_open(name, O_CREAT | O_RDWR, 0600);
    if (fd < 0) return DV_ERR_STATE;
    const int tr = ftruncate(fd, sizeof(IpcShm));
    void *mp = tr == 0 ? mmap(nullptr, sizeof(IpcShm), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
    close(fd);
    if (mp == MAP_FAILED) return DV_ERR_STATE;
    IpcXport *x = new IpcXport();
    x->shm = static_cast<IpcShm *>(mp);  // (a fresh segment is zero-filled: counters start at 0)
    x->P = nranks;
    x->r = rank;
    DvComm *m = new DvComm();
    m->nranks = nranks;
    m->rank = rank;
    m->x = x;
    auto fail = [&](int r) {
        comm_free(m);
        return r;
    };
    x->staging_cap = ipc_staging_bytes(cfg, (uint32_t)nranks);
    int r = alloc(&x->staging, x->staging_cap);
    if (!r) r = hip_fail2(hipIpcGetMemHandle(&x->shm->slot[rank].h, x->staging), "hipIpcGetMemHandle");
    if (r) return fail(r);
    x->shm->slot[rank].staging_bytes = x->staging_cap;
    x->shm->slot[rank].device = cfg.device;
    x->shm->joined.fetch_add(1, std::memory_order_acq_rel);
    r = x->barrier();  // every handle published
    for (int q = 0; q < nranks && !r; q++) {
        if (q == rank) {
            x->peer[q] = x->staging;
            continue;
        }
        void *p = nullptr;
        r = hip_fail2(hipIpcOpenMemHandle(&p, x->shm->slot[q].h, hipIpcMemLazyEnablePeerAccess),
                      "hipIpcOpenMemHandle");
        x->peer[q] = static_cast<uint8_t *>(p);
    }
    if (!r) r = x->barrier();  // every rank opened its peers: the name can go
    if (!r && rank == 0) (void)shm_unlink(name);
    if (!r) r = reserve(m, cfg.max_acc, cfg.max_txn, cfg.workload == DV_TPCC);
    if (r) return fail(r);
    slot = m;
    return DV_OK;
}

int dv_comm_init_local(dv_ctx **ctxs, int nranks) {
    if (!ctxs || nranks < 1 || nranks > kMaxLocalRanks) return DV_ERR_ARG;
    for (int q = 0; q < nranks; q++) {
        if (!ctxs[q]) return DV_ERR_ARG;
        const dv_config &cfg = ctx_config(ctxs[q]);
        if ((int)cfg.part_cnt != nranks || (int)cfg.part_id != q) return DV_ERR_ARG;
    }
    LocalGroup *g = new LocalGroup();
    g->P = nranks;
    g->slot.resize(nranks);
    int r = DV_OK;
    for (int q = 0; q < nranks && !r; q++) {
        dv_ctx *c = ctxs[q];
        r = hip_fail2(hipSetDevice(ctx_config(c).device), "hipSetDevice");
        if (!r) r = hip_fail2(hipEventCreateWithFlags(&g->slot[q].ready, hipEventDisableTiming), "event");
        if (!r) r = hip_fail2(hipEventCreateWithFlags(&g->slot[q].done, hipEventDisableTiming), "event");
        if (r) break;
        DvComm *&slot = ctx_comm(c);
        comm_free(slot);
        slot = new DvComm();
        slot->nranks = nranks;
        slot->rank = q;
        LocalXport *x = new LocalXport();
        x->g = g;
        x->r = q;
        g->refs++;
        slot->x = x;
        r = reserve(slot, ctx_config(c).max_acc, ctx_config(c).max_txn, ctx_config(c).workload == DV_TPCC);
    }
    if (g->refs == 0) {  // nothing handed out
        for (auto &sl : g->slot) {
            if (sl.ready) (void)hipEventDestroy(sl.ready);
            if (sl.done) (void)hipEventDestroy(sl.done);
        }
        delete g;
    }
    return r;
}

}  // extern "C"

namespace {

// device words -> the host: queue the mailbox kernel and spin on its
// sequence word (a drained stream without it is an error)
int mail_get(DvComm *m, hipStream_t s, const uint64_t *a, uint32_t na, const uint32_t *b, uint32_t nb,
             uint64_t *out64, uint32_t *out32, const uint64_t *c = nullptr, uint32_t nc = 0,
             uint64_t *outc = nullptr) {
    const unsigned long long want = ++m->mseq;
    DV_LAUNCH(k_mail_out, 1, kBlock, 0, s, a, na, b, nb, c, nc, m->d_mail, want);
    CHK(hip_fail2(hipGetLastError(), "k_mail_out"));
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t i = 0;; i++) {
        if (__atomic_load_n(&m->h_mail->seq, __ATOMIC_ACQUIRE) >= want) break;
        if ((i & 1023) == 1023) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess && __atomic_load_n(&m->h_mail->seq, __ATOMIC_ACQUIRE) >= want) break;
            if (q == hipSuccess) return hip_fail2(hipErrorUnknown, "mailbox");
            if (q != hipErrorNotReady) return hip_fail2(q, "stream");
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) return DV_ERR_STATE;
        }
        __builtin_ia32_pause();
    }
    for (uint32_t i = 0; i < na; i++) out64[i] = m->h_mail->w[i];
    for (uint32_t i = 0; i < nb; i++) out32[i] = (uint32_t)m->h_mail->w[na + i];
    for (uint32_t i = 0; i < nc; i++) outc[i] = m->h_mail->w[na + nb + i];
    return DV_OK;
}

// host words -> device buffers, as kernel arguments
int put_words(hipStream_t s, const uint64_t *v64, uint32_t n64, uint64_t *d64, const uint32_t *v32, uint32_t n32,
              uint32_t *d32) {
    PutArgs a{};
    a.n64 = n64;
    a.n32 = n32;
    a.d64 = d64;
    a.d32 = d32;
    for (uint32_t i = 0; i < n64 && i < (uint32_t)kRadix + 8; i++) a.v64[i] = v64[i];
    for (uint32_t i = 0; i < n32 && i < 8u; i++) a.v32[i] = v32[i];
    DV_LAUNCH(k_put_words, 1, kBlock, 0, s, a);
    return hip_fail2(hipGetLastError(), "k_put_words");
}

// The partitioned epoch of one rank (dv_epoch_run_part, dv_tpcc_epoch_run_part).
// No rank may leave between collectives on its own: arguments are voted on
// with the other ranks before anything depends on them, input errors found by
// the probe are combined before the rounds (every rank then reports the error
// at the same round), and the round loop's own exits depend only on combined
// verdicts, identical on every rank.  Only a missing context or communicator
// returns at once (no rank of this communicator can have entered a collective
// of it).  TPC-C (tpcc): records route by the owner bytes, carry their table
// and operation word, the epoch runs through dv_tpcc_epoch_begin, and the
// o_ids -- computed where the district row lives -- are all-reduced (MAX)
// into every rank's d_oid: Calvin's RFWD of o_id to the other participants
// (tpcc_txn.cpp:1040, txn.cpp:960-972, transport/message.cpp:982-1025), for every protocol.
// Replicated epochs in position-major order (DV_COMM_POSITION_ORDER; NO_WAIT
// / WAIT_DIE / OCC): the batches are all-gathered as row id | wr << 31 and
// position-major txn ids (origin q's txn j is j * P + q), interleaved txn by
// txn into the sequence order the E-schedule decides in -- the epoch groups'
// k_il_bounds / k_il_begin / k_il_move -- and decided by every rank with the
// single-GPU path; the commit bytes go back to origin order (k_il_commits).
// A malformed batch (txn ids not rising, past txns_per_rank) is not moved and
// every rank -- each interleaves the same gathered batches -- reads the
// refusal and returns DV_ERR_TXN_RANGE before anything is decided.  Why: the prefix
// of a prefix-kill epoch (the first n / 32 txns) then holds every origin's
// first txns and kills in every partition.
int run_part_position(dv_ctx *c, DvComm *m, const dv_epoch_dev *home, uint64_t n_home,
                      const std::vector<uint64_t> &recvc, uint64_t total, uint32_t txns_per_rank, uint32_t n_txn,
                      uint32_t max_len, uint8_t *d_commit, dv_stats *st) {
    const uint32_t P = (uint32_t)m->nranks;
    hipStream_t s = ctx_stream(c);
    uint8_t *sb = reinterpret_cast<uint8_t *>(m->send), *rb = reinterpret_cast<uint8_t *>(m->recv);
    uint32_t *sk = reinterpret_cast<uint32_t *>(sb), *stx = reinterpret_cast<uint32_t *>(sb + 4 * m->acc_cap);
    uint32_t *rk = reinterpret_cast<uint32_t *>(rb), *rt = reinterpret_cast<uint32_t *>(rb + 4 * m->acc_cap);
    if (n_home)
        DV_LAUNCH(k_group_pack, (uint32_t)std::min<uint64_t>((n_home + kBlock - 1) / kBlock, 2048), kBlock, 0, s,
                  home->keys, home->types, home->acc_txn, n_home, txns_per_rank, P, (uint32_t)m->rank, sk, stx);
    CHK(hip_fail2(hipGetLastError(), "pack"));
    uint64_t hmax = 0;
    bool equal = true;
    for (uint32_t q = 0; q < P; q++) {
        hmax = std::max<uint64_t>(hmax, recvc[q]);
        equal &= recvc[q] == recvc[0];
    }
    CHK(m->x->all_gather(reinterpret_cast<const uint8_t *>(sk), 4 * hmax, reinterpret_cast<uint8_t *>(rk), s));
    CHK(m->x->all_gather(reinterpret_cast<const uint8_t *>(stx), 4 * hmax, reinterpret_cast<uint8_t *>(rt), s));
    if (!equal) {  // (the padded parts packed, origin after origin)
        uint32_t *ck = reinterpret_cast<uint32_t *>(m->keys), *ct = m->txn;
        const dim3 grid((uint32_t)std::min<uint64_t>((hmax + kBlock - 1) / kBlock, 1024), std::min<uint32_t>(P, 64));
        DV_LAUNCH(k_rep_compact, grid, kBlock, 0, s, rk, rt, (const uint8_t *)nullptr, hmax, m->xcnt + P, P, ck, ct,
                  (uint8_t *)nullptr);
        CHK(hip_fail2(hipGetLastError(), "compact"));
        rk = ck;
        rt = ct;
    }
    XSegs xs{};
    xs.P = P;
    xs.tpr = txns_per_rank;
    uint64_t ro = 0;
    uint32_t xtiles = 0;
    for (uint32_t q = 0; q < P; q++) {
        xs.eoff[q] = ro;
        xs.toff[q] = xtiles;
        xtiles += (uint32_t)((recvc[q] + kXTile - 1) / kXTile);
        ro += recvc[q];
    }
    xs.eoff[P] = ro;
    xs.toff[P] = xtiles;
    xs.mP = div_magic(P);
    xs.mT = div_magic(txns_per_rank);
    const uint64_t nt = (uint64_t)P * txns_per_rank;
    CHK(hip_fail2(hipMemsetAsync(m->gbad, 0, sizeof(uint32_t), s), "memset"));
    if (!xtiles) {  // (no accesses: every txn empty)
        CHK(hip_fail2(hipMemsetAsync(m->iltb, 0, 4 * (nt + 1), s), "memset"));
    } else {
        DV_LAUNCH(k_il_bounds, (uint32_t)std::min<uint64_t>((nt + P + kBlock - 1) / kBlock, 4096), kBlock, 0, s, rt, xs,
                  m->tbo, m->ncnt);
        DV_LAUNCH(k_il_begin, (uint32_t)std::min<uint64_t>((nt + kBlock) / kBlock, 4096), kBlock, 0, s, xs, m->tbo,
                  m->ncnt, m->iltb, m->ilsh, (uint32_t *)nullptr);
        DV_LAUNCH(k_il_move<true>, xtiles, kBlock, 0, s, rk, rt, xs, m->ilsh, m->iltb, ro, m->ilk, m->ilt, m->gbad);
    }
    CHK(hip_fail2(hipGetLastError(), "k_il_move"));
    // every rank moved the same gathered batches, so every rank reads the
    // same refusal here and returns the same error -- no collective needed
    uint32_t refused = 0;
    CHK(mail_get(m, s, nullptr, 0, m->gbad, 1, nullptr, &refused));
    if (refused) return DV_ERR_TXN_RANGE;
    dv_epoch_dev ep{};
    ep.keys = reinterpret_cast<const uint64_t *>(m->ilk);  // (read as 32-bit row ids with the write bit)
    ep.types = nullptr;
    ep.acc_txn = m->ilt;
    ep.tables = nullptr;
    ep.n_acc = total;
    ep.n_txn = n_txn;
    ep.max_txn_acc = max_len;
    const int r = epoch_run_replicated(c, &ep, m->ilk, P, d_commit ? m->verdict : nullptr, st);
    if (r || !d_commit) return r;
    DV_LAUNCH(k_il_commits, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nt + kBlock - 1) / kBlock, 2048)),
              kBlock, 0, s, m->verdict, xs, d_commit);
    CHK(hip_fail2(hipGetLastError(), "k_il_commits"));
    return hip_fail2(hipStreamSynchronize(s), "sync");
}

int run_part(dv_ctx *c, const dv_epoch_dev *home, const uint8_t *own, const uint64_t *args, bool tpcc,
             uint32_t txns_per_rank, uint8_t *d_commit, uint64_t *d_oid, dv_stats *st) {
    if (!c) return DV_ERR_ARG;
    DvComm *m = ctx_comm(c);
    if (!m) return DV_ERR_STATE;
    const dv_config &cfg = ctx_config(c);
    const uint32_t P = (uint32_t)m->nranks;
    const uint64_t n_txn64 = (uint64_t)txns_per_rank * P;
    bool bad = !home || (home->n_acc && (!home->keys || !home->types || !home->acc_txn)) ||
               home->n_txn > txns_per_rank || n_txn64 > cfg.max_txn || n_txn64 > m->txn_cap ||
               home->n_acc > m->acc_cap || !ctx_has_tables(c) || tpcc != (cfg.workload == DV_TPCC);
    if (tpcc && !bad) bad = home->n_acc && (!home->tables || !own || !args || !m->send_args);
    if (!bad && home->ts && cfg.cc_alg == DV_WAIT_DIE) bad = true;  // (dvcc.h: partitioned epochs take no ts)
    const uint32_t n_txn = bad ? 0u : (uint32_t)n_txn64;
    const uint64_t n_home = bad ? 0 : home->n_acc;
    hipStream_t s = ctx_stream(c);
    const uint32_t nb = n_home ? nblocks_for(n_home) : 1;

    // 1. the first vote -- longest txn (the verdict-byte stride on every
    //    rank), bad arguments, longest batch, what blocks a replicated epoch
    //    -- and every rank's batch size
    const bool rep_here = !tpcc && m->mode != 1 && ctx_rep_capable(c, P);
    // (and the sequence order: a replicated epoch may merge the origins' batches
    // txn by txn, DV_COMM_POSITION_ORDER -- every rank the same order, else
    // DV_ERR_ARG on every rank)
    const uint32_t vote[6] = {(!bad && home->max_txn_acc) ? home->max_txn_acc : kMaxPos, bad ? kVoteBadArg : 0u,
                              (uint32_t)std::min<uint64_t>(n_home, 0xFFFFFFFFull), rep_here ? 0u : kRepBlockOff,
                              m->position ? 1u : 0u, m->position ? 0u : 1u};
    std::vector<uint64_t> sendc(P, n_home), recvc(P);
    CHK(put_words(s, sendc.data(), P, m->xcnt, vote, 6, m->xvote));
    CHK(m->x->all_to_all_u64(m->xcnt, m->xcnt + P, s));
    CHK(m->x->max_u32(m->xvote, 6, s));
    uint32_t gvote[6] = {0, 0, 0, 0, 0, 0};
    CHK(mail_get(m, s, m->xcnt + P, P, m->xvote, 6, recvc.data(), gvote));
    if (gvote[1] || (gvote[4] && gvote[5])) return DV_ERR_ARG;  // every rank: bad arguments, or mixed orders
    const uint32_t max_len = std::min<uint32_t>(gvote[0], kMaxPos);
    // 2. replicated when every rank allows it and the whole epoch fits this
    //    context (the same decision on every rank: voted and gathered values)
    const uint64_t cap = std::min<uint64_t>(cfg.max_acc, m->acc_cap);
    uint64_t total = 0;
    for (uint32_t q = 0; q < P; q++) total += recvc[q];
    //    (one rank too: the replicated epoch is the single-GPU path plus a
    //    local copy, the list protocol a host round trip per decision round)
    // position-major replicated epochs: the write bit in bit 31 of the row ids
    // (global keys below 2^31), as the epoch groups' batches
    const bool il = gvote[4] && cfg.cc_alg != DV_CALVIN && P > 1 && P <= kXMaxP && ctx_table0_rows(c) * P < (1ull << 31);
    if (!gvote[3] && total <= cap && (uint64_t)gvote[2] * P <= m->acc_cap && il)
        return run_part_position(c, m, home, n_home, recvc, total, txns_per_rank, n_txn, max_len, d_commit, st);
    if (!gvote[3] && total <= cap && (uint64_t)gvote[2] * P <= m->acc_cap) {
        // send and receive areas: [row ids 4 B | txn ids 4 B | types 1 B] per access
        uint8_t *sb = reinterpret_cast<uint8_t *>(m->send), *rb = reinterpret_cast<uint8_t *>(m->recv);
        uint32_t *sk = reinterpret_cast<uint32_t *>(sb), *st_ = reinterpret_cast<uint32_t *>(sb + 4 * m->acc_cap);
        uint8_t *sy = sb + 8 * m->acc_cap;
        uint32_t *rk = reinterpret_cast<uint32_t *>(rb), *rt = reinterpret_cast<uint32_t *>(rb + 4 * m->acc_cap);
        uint8_t *ry = rb + 8 * m->acc_cap;
        if (n_home)
            DV_LAUNCH(k_rep_pack, std::min<uint32_t>(nb * 16, 2048), kBlock, 0, s, home->keys, home->types, home->acc_txn,
                                                                             n_home, txns_per_rank, (uint32_t)m->rank * txns_per_rank,
                                                                             sk, st_, sy);
        CHK(hip_fail2(hipGetLastError(), "pack"));
        // one all-gather per array, parts padded to the longest batch; equal
        // batches (the usual case) land contiguous, others are packed after
        uint64_t hmax = 0;
        bool equal = true;
        for (uint32_t q = 0; q < P; q++) {
            hmax = std::max<uint64_t>(hmax, recvc[q]);
            equal &= recvc[q] == recvc[0];
        }
        CHK(m->x->all_gather(reinterpret_cast<const uint8_t *>(sk), 4 * hmax, reinterpret_cast<uint8_t *>(rk), s));
        CHK(m->x->all_gather(reinterpret_cast<const uint8_t *>(st_), 4 * hmax, reinterpret_cast<uint8_t *>(rt), s));
        CHK(m->x->all_gather(sy, hmax, ry, s));
        if (!equal) {
            uint32_t *ck = reinterpret_cast<uint32_t *>(m->keys), *ct = m->txn;
            const dim3 grid((uint32_t)std::min<uint64_t>((hmax + kBlock - 1) / kBlock, 1024), std::min<uint32_t>(P, 64));
            DV_LAUNCH(k_rep_compact, grid, kBlock, 0, s, rk, rt, ry, hmax, m->xcnt + P, P, ck, ct, m->types);
            CHK(hip_fail2(hipGetLastError(), "compact"));
            rk = ck;
            rt = ct;
            ry = m->types;
        }
        dv_epoch_dev ep{};
        ep.keys = reinterpret_cast<const uint64_t *>(rk);  // (read as 32-bit row ids)
        ep.types = ry;
        ep.acc_txn = rt;
        ep.tables = nullptr;
        ep.n_acc = total;
        ep.n_txn = n_txn;
        ep.max_txn_acc = max_len;
        return epoch_run_replicated(c, &ep, rk, P, d_commit, st);
    }
    // 3. the list protocol: split the batch by owner (a bad rank sends nothing).
    //    Position-major (the vote's order flag; not CALVIN, whose order is the
    //    sequencer's): origin q's txn j is sequence number j * P + q, as in the
    //    epoch groups and the replicated epochs
    const bool ilist = gvote[4] && cfg.cc_alg != DV_CALVIN && P > 1 && P <= kXMaxP;
    if (n_home) {
        DV_LAUNCH(k_owner_count, nb, kBlock, 0, s, home->keys, own, n_home, P, m->counts, nb, m->xvote);
        DV_LAUNCH(k_owner_scan, P, kBlock, 0, s, m->counts, nb, m->tot);
        DV_LAUNCH(k_owner_scatter, nb, kBlock, 0, s, home->keys, home->types, home->acc_txn, own,
                                             tpcc ? home->tables : nullptr, args, n_home, P, txns_per_rank,
                                             ilist ? (uint32_t)m->rank : (uint32_t)m->rank * txns_per_rank,
                                             ilist ? P : 1u, m->counts, m->tot, nb, m->send,
                                             tpcc ? m->send_args : nullptr, m->xvote);
    } else {
        CHK(hip_fail2(hipMemsetAsync(m->tot, 0, P * sizeof(uint32_t), s), "memset"));
    }
    CHK(hip_fail2(hipGetLastError(), "owner split"));
    // per-owner counts, the second vote (owner bytes, capacity), the records
    std::vector<uint32_t> tot(P);
    CHK(mail_get(m, s, nullptr, 0, m->tot, P, nullptr, tot.data()));
    for (uint32_t o = 0; o < P; o++) sendc[o] = tot[o];
    CHK(put_words(s, sendc.data(), P, m->xcnt, nullptr, 0, nullptr));
    CHK(m->x->all_to_all_u64(m->xcnt, m->xcnt + P, s));
    DV_LAUNCH(k_recv_check, 1, 64, 0, s, m->xcnt + P, P, cap, m->xvote);
    CHK(m->x->max_u32(m->xvote, 2, s));
    CHK(mail_get(m, s, m->xcnt + P, P, m->xvote, 2, recvc.data(), gvote));
    if (gvote[1]) return DV_ERR_ARG;  // every rank: some rank's owner bytes or capacity were bad
    std::vector<size_t> sc(P), sd(P), rc(P), rd(P);
    uint64_t n_recv = 0, so = 0;
    for (uint32_t o = 0; o < P; o++) {
        sc[o] = sendc[o] * sizeof(dv_access);
        sd[o] = so * sizeof(dv_access);
        so += sendc[o];
        rc[o] = recvc[o] * sizeof(dv_access);
        rd[o] = n_recv * sizeof(dv_access);
        n_recv += recvc[o];
    }
    CHK(m->x->all_to_allv(reinterpret_cast<const uint8_t *>(m->send), sc.data(), sd.data(),
                          reinterpret_cast<uint8_t *>(m->recv), rc.data(), rd.data(), s));
    if (tpcc) {  // the operation words: the same segments at 8 bytes per record
        std::vector<size_t> sc8(P), sd8(P), rc8(P), rd8(P);
        for (uint32_t o = 0; o < P; o++) {
            sc8[o] = sc[o] / sizeof(dv_access) * 8;
            sd8[o] = sd[o] / sizeof(dv_access) * 8;
            rc8[o] = rc[o] / sizeof(dv_access) * 8;
            rd8[o] = rd[o] / sizeof(dv_access) * 8;
        }
        CHK(m->x->all_to_allv(reinterpret_cast<const uint8_t *>(m->send_args), sc8.data(), sd8.data(),
                              reinterpret_cast<uint8_t *>(m->recv_args), rc8.data(), rd8.data(), s));
    }
    CHK(hip_fail2(hipMemsetAsync(m->err, 0, 4, s), "memset"));
    XSegs xs{};
    const uint64_t *recv_args = tpcc ? m->recv_args : nullptr;
    if (ilist) {  // the records split into the epoch's arrays in sequence order (k_ilist_move)
        xs.P = P;
        xs.tpr = txns_per_rank;
        xs.mP = div_magic(P);
        xs.mT = div_magic(txns_per_rank);
        uint64_t off = 0;
        for (uint32_t q = 0; q < P; q++) {
            xs.eoff[q] = off;
            off += recvc[q];
        }
        xs.eoff[P] = off;
        const uint64_t nt = (uint64_t)P * txns_per_rank;
        DV_LAUNCH(k_ilist_bounds, (uint32_t)std::min<uint64_t>((nt + P + kBlock - 1) / kBlock, 4096), kBlock, 0, s,
                  reinterpret_cast<const dv_access *>(m->recv), xs, m->tbo, m->ncnt);
        DV_LAUNCH(k_il_begin, (uint32_t)std::min<uint64_t>((nt + kBlock) / kBlock, 4096), kBlock, 0, s, xs, m->tbo,
                  m->ncnt, m->iltb, m->ilsh, (uint32_t *)nullptr);
        if (n_recv)
            DV_LAUNCH(k_ilist_move, (uint32_t)std::min<uint64_t>((n_recv + kBlock - 1) / kBlock, 4096), kBlock, 0, s,
                      reinterpret_cast<const dv_access *>(m->recv), recv_args, xs, m->ilsh, m->iltb, n_recv, m->keys,
                      m->types, m->txn, m->tables, tpcc ? m->send_args : nullptr, m->err);
        if (tpcc) recv_args = m->send_args;  // (the send area is free once the records have landed)
    } else {
        launch_split_access(s, m->recv, n_recv, nullptr, n_txn, m->keys, m->types, m->txn, m->tables, m->err);
    }
    CHK(hip_fail2(hipGetLastError(), "unpack"));

    // 3. the partition's epoch: input errors combined, then the rounds closed
    //    by list all-reduces
    dv_epoch_dev ep{};
    ep.keys = m->keys;
    ep.types = m->types;
    ep.acc_txn = m->txn;
    ep.tables = tpcc ? m->tables : nullptr;
    ep.n_acc = n_recv;
    ep.n_txn = n_txn;
    ep.max_txn_acc = max_len;
    // (position-major: the o_id land by sequence number and go back to origin order after the all-reduce)
    uint64_t *oid = ilist && d_oid ? m->iloid : d_oid;
    if (tpcc) {
        CHK(dv_tpcc_epoch_begin(c, &ep, recv_args, oid));
    } else {
        CHK(dv_epoch_begin(c, &ep, nullptr));
    }
    if (ilist) {  // a record the interleave refused rejects the epoch on every rank (the combine below)
        DV_LAUNCH(k_refusal_err, 1, 64, 0, s, ctx_err_words(c), (const uint32_t *)m->err);
        CHK(hip_fail2(hipGetLastError(), "k_refusal_err"));
    }
    CHK(dv_epoch_errors_local(c, m->gerr));
    CHK(m->x->max_u32(m->gerr, 1, s));
    CHK(dv_epoch_errors_combined(c, m->gerr));
    if (cfg.cc_alg != DV_CALVIN) {
        constexpr uint32_t kLag = 2;  // rounds queued ahead of the outcome read
        std::vector<uint32_t> counts{n_txn};  // list length entering each known round
        uint32_t r = 0;
        while (counts.back() > 0) {
            CHK(dv_epoch_round_local(c, m->verdict));
            CHK(m->x->max_u8(m->verdict, counts.back(), s));
            CHK(dv_epoch_round_apply(c, m->verdict, nullptr));
            if (++r >= kLag) {
                uint32_t und = 0;
                // an input error anywhere: every rank returns it here, at the same round
                CHK(dv_epoch_round_wait(c, r - kLag, &und));
                // the combined verdicts are the same on every rank, so is und
                if (und != 0 && und >= counts.back()) return DV_ERR_STATE;  // every round decides one
                counts.push_back(und);
            }
        }
    }
    // 4. execute and report (CALVIN: a rejected epoch executes nothing, and
    //    every rank reports the combined error); the errors are combined, so
    //    every rank takes the o_id all-reduce or none does
    const int r = dv_epoch_finish(c, ilist && d_commit ? m->verdict : d_commit, st);
    if (r) return r;
    const uint32_t ilg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n_txn + kBlock - 1) / kBlock, 2048));
    if (ilist && d_commit && n_txn) {  // (commit bytes back in origin order)
        DV_LAUNCH(k_il_commits, ilg, kBlock, 0, s, m->verdict, xs, d_commit);
        CHK(hip_fail2(hipGetLastError(), "k_il_commits"));
    }
    if (!tpcc || !d_oid || !n_txn) return ilist && d_commit ? hip_fail2(hipStreamSynchronize(s), "sync") : DV_OK;
    CHK(m->x->max_u64(oid, n_txn, s));
    if (ilist) {
        DV_LAUNCH(k_il_words, ilg, kBlock, 0, s, m->iloid, xs, d_oid);
        CHK(hip_fail2(hipGetLastError(), "k_il_words"));
    }
    return hip_fail2(hipStreamSynchronize(s), "sync");
}


// One epoch group (dv_epoch_group_run): homes[e] is this rank's client batch
// of epoch e of the group.  Collectives, in the same order on every rank:
//   1. all-to-all of the batch sizes (rank e learns the parts of epoch e) and
//      the argument vote (all-reduce MAX);
//   2. two all-to-allv (grouped) move every batch to its epoch's decider as
//      8 B per access -- row id with the write bit, global txn id -- landing
//      contiguous in origin order, Calvin's sequence (work_queue.cpp:105-151);
//   3. rank e decides epoch e with the replicated single-GPU path (prefix
//      kill, asynchronous rounds; its one all-reduce of the input-error bits
//      after the probe fails the group on every rank), routing the committed
//      accesses by owner instead of executing them;
//   4. all-to-all of {committed txns, records per owner} and the outcome vote;
//   5. two all-to-allv (grouped): the records to their owners (RFWD-like
//      forwarding of what each owner must write, message.cpp:982-1025), and
//      every origin's commit bytes back to it (the client responses);
//   6. each rank executes the records of epochs 0..P-1 on its rows, in order.
// Groups run back to back (dv_epoch_group_run_batch) leave their execution
// digest on the device (defer) and the next group's vote reads it in the same
// mailbox trip: the host then waits once between two groups, not twice.
struct GroupDefer {
    dv_stats *st = nullptr;  // the group whose read digest / write count are still on the device
};
void group_digest(dv_stats *st, const uint64_t *slots) {
    uint64_t acc[2] = {0, 0};
    for (int k = 0; k < kSlots; k++) {
        acc[0] += slots[2 * k];
        acc[1] += slots[2 * k + 1];
    }
    st->read_digest = acc[0];
    st->write_cnt = acc[1];
}
int run_group(dv_ctx *c, const dv_epoch_dev *homes, uint32_t n_homes, uint32_t txns_per_rank, uint8_t *d_commit,
              dv_stats *st, GroupDefer *dfr = nullptr, bool defer = false) {
    if (!c) return DV_ERR_ARG;
    DvComm *m = ctx_comm(c);
    if (!m) return DV_ERR_STATE;
    const dv_config &cfg = ctx_config(c);
    const uint32_t P = (uint32_t)m->nranks;
    const uint64_t n_txn64 = (uint64_t)txns_per_rank * P;
    bool bad = !homes || n_homes != P || n_txn64 > cfg.max_txn || n_txn64 > m->txn_cap || !ctx_has_tables(c) ||
               cfg.workload != DV_YCSB;
    uint64_t n_send = 0;
    uint32_t max_len = 0;
    for (uint32_t e = 0; e < P && !bad; e++) {
        const dv_epoch_dev &h = homes[e];
        bad = h.n_txn > txns_per_rank || (h.n_acc && (!h.keys || !h.types || !h.acc_txn)) ||
              (h.ts && cfg.cc_alg == DV_WAIT_DIE) || (h.n_acc >> 32) != 0;
        n_send += h.n_acc;
        if (h.n_acc) max_len = std::max<uint32_t>(max_len, h.max_txn_acc ? h.max_txn_acc : kMaxPos);
    }
    bad = bad || n_send > m->acc_cap;
    hipStream_t s = ctx_stream(c);
    const uint64_t acap = m->acc_cap;

    // 1. one all-gather of every rank's vote record -- longest txn, bad
    //    arguments, "not a dense YCSB map" (then nobody runs), table rows
    //    (all equal, so a key's range check on its decider is its owner's
    //    check), receive capacity, then its batch size per epoch -- from which
    //    every rank derives the same decision and its receive sizes
    const bool capable = ctx_group_capable(c, P);
    uint64_t *f0 = nullptr;
    const uint64_t *pkey = nullptr;
    const uint32_t W = kGroupRecHead + P;
    std::vector<uint64_t> rec(W, 0), all((size_t)P * W), sendc(P, 0), recvc(P);
    rec[0] = max_len;
    rec[1] = bad ? 1u : 0u;
    rec[2] = capable ? 0u : 1u;
    rec[3] = capable ? ctx_table0_rows(c) : 0u;
    rec[4] = std::min<uint64_t>(cfg.max_acc, acap);
    // compact batches (k_group_pack_c) need the global row ids below 2^30
    rec[5] = capable && !m->wide && P <= kXMaxP && ctx_table0_rows(c) * P < (1ull << 30) ? 0u : 1u;
    // position-major sequence (DV_COMM_POSITION_ORDER; CALVIN keeps its origin order)
    const bool il = m->position && cfg.cc_alg != DV_CALVIN && P > 1 && P <= kXMaxP;  // (one origin: the same order)
    rec[6] = il ? 1u : 0u;
    // tbx: every batch brings its txn_begin and the decider will take tb mode
    // (a prefix-kill epoch) -- the boundaries travel, nothing is renumbered
    bool has_tb = m->tbr != nullptr;
    for (uint32_t e = 0; e < P && !bad; e++) has_tb &= homes[e].txn_begin != nullptr || homes[e].n_txn == 0;
    {
        dv_epoch_dev probe{};
        probe.n_txn = (uint32_t)n_txn64;
        probe.txn_begin = m->iltb;
        probe.recs32 = m->ilk;
        has_tb = has_tb && group_tb_epoch(c, &probe);
    }
    rec[7] = has_tb ? 1u : 0u;
    // per epoch: the batch's accesses, and above bit 32 the words of its
    // txn_begin it would send (tbx: n_txn + 1 straight from its buffer)
    for (uint32_t e = 0; e < P && !bad; e++) {
        sendc[e] = homes[e].n_acc;
        rec[kGroupRecHead + e] = sendc[e] | (uint64_t)(homes[e].txn_begin ? homes[e].n_txn + 1u : 0u) << 32;
    }
    // (and the compact pack's bad flag cleared for this group: a group that
    // failed after setting it must not leave it to the next one)
    const uint32_t zero = 0;
    CHK(put_words(s, rec.data(), W, m->gs, &zero, 1, m->gbad));
    CHK(m->x->all_gather(reinterpret_cast<const uint8_t *>(m->gs), 8ull * W, reinterpret_cast<uint8_t *>(m->gr), s));
    {
        // (with the previous group's execution digest, when it was deferred)
        dv_stats *prev = dfr ? dfr->st : nullptr;
        uint64_t pslots[2 * kSlots];
        CHK(mail_get(m, s, m->gr, P * W, nullptr, 0, all.data(), nullptr,
                     prev ? reinterpret_cast<const uint64_t *>(m->xacc) : nullptr, prev ? 2 * kSlots : 0, pslots));
        if (prev) {
            group_digest(prev, pslots);
            dfr->st = nullptr;
        }
    }
    uint64_t gmax = 0;
    bool refuse = false, compact = true, tbx = true;
    std::vector<uint32_t> rtbw(P);  // words of txn_begin origin q sends for this rank's epoch
    for (uint32_t q = 0; q < P; q++) {
        const uint64_t *r = &all[(size_t)q * W];
        gmax = std::max<uint64_t>(gmax, r[0]);
        compact &= r[5] == 0;
        tbx &= r[7] == 1;
        refuse |= r[1] || r[2] || r[3] != all[3] || r[6] != all[6];  // (every rank the same order)
        uint64_t in = 0;  // what rank q receives: its epoch's batches
        for (uint32_t o = 0; o < P; o++) in += all[(size_t)o * W + kGroupRecHead + q] & 0xFFFFFFFFull;
        refuse |= in > r[4];
        recvc[q] = r[kGroupRecHead + m->rank] & 0xFFFFFFFFull;
        rtbw[q] = (uint32_t)(r[kGroupRecHead + m->rank] >> 32);
    }
    if (refuse) return DV_ERR_ARG;  // every rank
    tbx = tbx && compact;
    const uint32_t glen = (uint32_t)std::min<uint64_t>(gmax ? gmax : 1u, kMaxPos);

    // 2. every batch to its decider: [row id | wr << 31, 4 B | txn id, 4 B],
    //    or compact: [row id | start << 30 | wr << 31, 4 B] and the txn ids
    //    numbered again on the decider
    uint8_t *sb = reinterpret_cast<uint8_t *>(m->send), *rb = reinterpret_cast<uint8_t *>(m->recv);
    uint32_t *sk = reinterpret_cast<uint32_t *>(sb), *stx = reinterpret_cast<uint32_t *>(sb + 4 * acap);
    uint32_t *rk = reinterpret_cast<uint32_t *>(rb), *rt = reinterpret_cast<uint32_t *>(rb + 4 * acap);
    std::vector<size_t> sc(P), sd(P), rc(P), rd(P);
    uint64_t so = 0, ro = 0;
    XSegs xs{};
    xs.P = P;
    xs.tpr = txns_per_rank;
    uint32_t xtiles = 0;
    PackSrc ps{};
    uint64_t nmax = 0;
    for (uint32_t e = 0; e < P; e++) {
        const uint64_t n = sendc[e];
        if (compact) {
            ps.keys[e] = homes[e].keys;
            ps.types[e] = homes[e].types;
            ps.recs[e] = homes[e].recs32;
            ps.txn[e] = homes[e].acc_txn;
            ps.n[e] = n;
            ps.off[e] = so;
            ps.n_txn[e] = homes[e].n_txn;
            nmax = std::max(nmax, n);
        } else if (n) {
            const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + kBlock - 1) / kBlock, 2048);
            DV_LAUNCH(k_group_pack, blocks, kBlock, 0, s, homes[e].keys, homes[e].types, homes[e].acc_txn, n,
                      txns_per_rank, il ? P : 1u, il ? (uint32_t)m->rank : (uint32_t)m->rank * txns_per_rank,
                      sk + so, stx + so);
        }
        sc[e] = 4 * n;
        sd[e] = 4 * so;
        so += n;
        rc[e] = 4 * recvc[e];
        rd[e] = 4 * ro;
        if (compact || il) {
            xs.eoff[e] = ro;
            xs.toff[e] = xtiles;
            xtiles += (uint32_t)((recvc[e] + kXTile - 1) / kXTile);
        }
        ro += recvc[e];
    }
    // the batches' 4-byte records as they are (dv_epoch_dev::recs32, key | wr
    // << 31): with the boundaries travelling (tbx) the compact record is the
    // same word -- the pack would only saturate a key past 30 bits, which the
    // decider's range check refuses either way (rows * P < 2^30) -- so each
    // batch goes to the all-to-allv straight from its buffer
    bool direct = compact && tbx;
    for (uint32_t e = 0; e < P && direct; e++) direct = sendc[e] == 0 || homes[e].recs32 != nullptr;
    std::vector<const uint8_t *> segs(P);
    if (direct)
        for (uint32_t e = 0; e < P; e++) segs[e] = reinterpret_cast<const uint8_t *>(homes[e].recs32);
    if (compact && nmax && !direct) {
        const uint32_t bx = (uint32_t)std::min<uint64_t>((nmax + kBlock - 1) / kBlock, std::max(1u, 2048u / P));
        DV_LAUNCH(k_group_pack_c, dim3(bx, P), kBlock, 0, s, ps, sk, m->gbad, tbx ? 1 : 0);
    }
    // tbx: each batch's txn_begin straight from its buffer (n_txn + 1 words,
    // none for a batch without boundaries), landing at q * (tpr + 1); the
    // receiver checks them (k_tb_origin / k_il_begin)
    std::vector<size_t> bc(P), bcr(P), bdr(P);
    std::vector<const uint8_t *> tsegs(P);
    if (tbx)
        for (uint32_t e = 0; e < P; e++) {
            tsegs[e] = reinterpret_cast<const uint8_t *>(homes[e].txn_begin);
            bc[e] = homes[e].txn_begin ? 4ull * (homes[e].n_txn + 1) : 0;
            bcr[e] = 4ull * rtbw[e];
            bdr[e] = 4ull * (txns_per_rank + 1) * e;
            xs.tbw[e] = rtbw[e];
        }
    CHK(hip_fail2(hipGetLastError(), "pack"));
    CHK(m->x->group(true));
    if (direct)
        CHK(m->x->all_to_allv_segs(segs.data(), sc.data(), reinterpret_cast<uint8_t *>(rk), rc.data(), rd.data(), s));
    else
        CHK(m->x->all_to_allv(reinterpret_cast<const uint8_t *>(sk), sc.data(), sd.data(),
                              reinterpret_cast<uint8_t *>(rk), rc.data(), rd.data(), s));
    if (tbx)
        CHK(m->x->all_to_allv_segs(tsegs.data(), bc.data(), reinterpret_cast<uint8_t *>(m->tbr), bcr.data(),
                                   bdr.data(), s));
    if (!compact)
        CHK(m->x->all_to_allv(reinterpret_cast<const uint8_t *>(stx), sc.data(), sd.data(),
                              reinterpret_cast<uint8_t *>(rt), rc.data(), rd.data(), s));
    CHK(m->x->group(false));
    xs.eoff[P] = ro;
    xs.toff[P] = xtiles;
    xs.mP = div_magic(P);
    xs.mT = div_magic(txns_per_rank);
    if (compact && xtiles && !tbx) {
        DV_LAUNCH(k_group_txn_count, xtiles, kBlock, 0, s, rk, xs, m->gtc, il ? m->ncnt : nullptr);
        DV_LAUNCH(k_group_txn_ids, xtiles, kBlock, 0, s, rk, xs, m->gtc, rt, il ? m->tbo : nullptr,
                  il ? m->ncnt : nullptr);
        CHK(hip_fail2(hipGetLastError(), "k_group_txn_ids"));
    }
    // 3. decide this rank's epoch; its committed accesses are routed into the
    //    send area (free again once the batches have left)
    dv_epoch_dev ep{};
    ep.keys = reinterpret_cast<const uint64_t *>(rk);  // (read as 32-bit row ids with the write bit)
    ep.types = nullptr;
    ep.acc_txn = rt;
    ep.tables = nullptr;
    ep.n_acc = ro;
    ep.n_txn = (uint32_t)n_txn64;
    ep.max_txn_acc = glen;
    const uint32_t *ek = rk;
    const uint64_t ntx = (uint64_t)P * txns_per_rank;
    if (tbx && !il) {  // origin-major with the boundaries: the landed batches as they are, tb mode
        DV_LAUNCH(k_tb_origin, (uint32_t)std::min<uint64_t>((ntx + kBlock) / kBlock, 4096), kBlock, 0, s, xs, m->tbr,
                  m->iltb, m->gbad);
        CHK(hip_fail2(hipGetLastError(), "k_tb_origin"));
        ep.txn_begin = m->iltb;
        ep.recs32 = rk;
        ep.acc_txn = nullptr;
    } else if (tbx) {  // position-major with the boundaries: interleaved by txn tiles
        ek = m->ilk;
        ep.keys = reinterpret_cast<const uint64_t *>(ek);
        ep.txn_begin = m->iltb;
        ep.recs32 = ek;
        ep.acc_txn = nullptr;
        DV_LAUNCH(k_il_begin, (uint32_t)std::min<uint64_t>((ntx + kBlock) / kBlock, 4096), kBlock, 0, s, xs, m->tbr,
                  (const uint32_t *)nullptr, m->iltb, m->ilsh, m->gbad);
        const uint32_t tiles = (txns_per_rank + kIlTxns - 1) / kIlTxns;
        if (ro && tiles)
            DV_LAUNCH(k_il_move_tb, P * tiles, kBlock, 0, s, rk, xs, m->tbr, m->ilsh, ro, m->ilk, m->gbad);
        CHK(hip_fail2(hipGetLastError(), "k_il_move_tb"));
    } else if (il) {
        // position-major: the landed batches interleaved txn by txn, with the
        // epoch's boundaries -- a prefix-kill decider then reads those and the
        // 32-bit rows as its records (tb mode), no per-access txn ids
        ek = m->ilk;
        ep.keys = reinterpret_cast<const uint64_t *>(ek);
        ep.txn_begin = m->iltb;
        ep.recs32 = ek;
        const bool tb = group_tb_epoch(c, &ep);
        ep.acc_txn = tb ? nullptr : m->ilt;
        const uint64_t nt = (uint64_t)P * txns_per_rank;
        if (!xtiles) {  // (no accesses: every txn empty)
            CHK(hip_fail2(hipMemsetAsync(m->iltb, 0, 4 * (nt + 1), s), "memset"));
        } else {
            if (!compact)
                DV_LAUNCH(k_il_bounds, (uint32_t)std::min<uint64_t>((nt + P + kBlock - 1) / kBlock, 4096), kBlock, 0,
                          s, rt, xs, m->tbo, m->ncnt);
            DV_LAUNCH(k_il_begin, (uint32_t)std::min<uint64_t>((nt + kBlock) / kBlock, 4096), kBlock, 0, s, xs,
                      m->tbo, m->ncnt, m->iltb, m->ilsh, (uint32_t *)nullptr);
            if (compact)
                DV_LAUNCH(k_il_move<false>, xtiles, kBlock, 0, s, rk, rt, xs, m->ilsh, m->iltb, ro, m->ilk,
                          tb ? nullptr : m->ilt, m->gbad);
            else
                DV_LAUNCH(k_il_move<true>, xtiles, kBlock, 0, s, rk, rt, xs, m->ilsh, m->iltb, ro, m->ilk,
                          tb ? nullptr : m->ilt, m->gbad);
        }
        CHK(hip_fail2(hipGetLastError(), "k_il_move"));
    }
    bool rec_written = false;  // (the owner scan wrote the outcome record)
    RouteOut rout{reinterpret_cast<uint2 *>(m->send), m->rblk, m->rtot, P};
    rout.orec = m->gs;
    rout.bad = m->gbad;
    rout.xacc = m->xacc;
    rout.cap = 2 * acap;
    rout.ctr = ctx_counters(c);
    rout.wrote = &rec_written;
    // (CALVIN counts its commits after the route: its record needs the host)
    rout.defer = cfg.cc_alg != DV_CALVIN;
    dv_stats est{};
    int rd_ = epoch_run_replicated(c, &ep, ek, P, m->verdict, &est, &rout);
    // the decider's counters are still on their way (RouteOut::defer): the
    // outcome vote's round trip brings them, and a context left between the
    // two is finished before returning
    bool pending = rd_ == DV_OK && ctx_finish_pending(c);
    auto settle = [&]() {
        if (pending) {
            rd_ = epoch_replicated_complete(c, &est);
            pending = false;
        }
    };

    // 4. one all-gather of every rank's outcome record: a failure on any rank
    //    (or an owner whose receive area is too small) fails the group on
    //    every rank; committed txns; records per owner.  A decider whose
    //    rounds halted (record word 4) finishes them once the vote is in, and
    //    every rank votes again.
    uint64_t gfail = 0, committed = 0;
    for (int vote = 0;; vote++) {
        const uint32_t fail = rd_ ? (uint32_t)(-rd_) : 0u;
        if (rd_ || !rec_written) {
            DV_LAUNCH(k_route_words, 1, 64, 0, s, m->rtot, P, rd_ ? 0ull : est.committed, fail, 2 * acap, m->gs,
                      m->gbad, m->xacc);
            int e = hip_fail2(hipGetLastError(), "k_route_words");
            if (e) { settle(); return e; }
        }
        int e = m->x->all_gather(reinterpret_cast<const uint8_t *>(m->gs), 8ull * W, reinterpret_cast<uint8_t *>(m->gr), s);
        if (!e) e = mail_get(m, s, m->gr, P * W, nullptr, 0, all.data(), nullptr);
        settle();  // (its counters arrived with the vote)
        if (e) return e;
        gfail = committed = 0;
        bool refused = false, halted = false;
        for (uint32_t q = 0; q < P; q++) {
            const uint64_t *r = &all[(size_t)q * W];
            gfail = std::max<uint64_t>(gfail, r[0]);
            refused |= r[3] != 0;
            halted |= r[4] != 0;
            committed += r[1];
            uint64_t in = 0;
            for (uint32_t o = 0; o < P; o++) in += all[(size_t)o * W + kGroupRecHead + q];
            if (in > r[2]) gfail = std::max<uint64_t>(gfail, (uint64_t)(-DV_ERR_ARG));
        }
        // a batch its sender (or the move) refused makes the group an argument
        // error on every rank, whatever the deciders made of it
        if (refused) gfail = (uint64_t)(-DV_ERR_ARG);
        if (gfail) return -(int)gfail;
        // (a finished decision is not halted again: a second one cannot happen)
        if (!halted) break;
        if (vote > 0) return DV_ERR_STATE;
    }
    // a decider whose finish failed after an outcome it voted as good (an
    // invariant the finish checks, or HIP itself): its peers go on
    if (rd_) return rd_;

    // 5. records to their owners, commit bytes back to their origins
    std::vector<uint64_t> rcnt(P);
    so = ro = 0;
    std::vector<size_t> tc(P), td(P), uc(P), ud(P);
    for (uint32_t q = 0; q < P; q++) {
        const uint64_t out = all[(size_t)m->rank * W + kGroupRecHead + q];
        const uint64_t in = all[(size_t)q * W + kGroupRecHead + m->rank];
        rcnt[q] = in;
        sc[q] = 8 * out;
        sd[q] = 8 * so;
        rc[q] = 8 * in;
        rd[q] = 8 * ro;
        so += out;
        ro += in;
        tc[q] = uc[q] = txns_per_rank;
        td[q] = (size_t)q * txns_per_rank;
        ud[q] = (size_t)q * txns_per_rank;
    }
    uint8_t *commit_out = d_commit ? d_commit : m->gcommit;
    const uint8_t *vsend = m->verdict;
    if (il) {  // (the commit bytes in origin order again)
        const uint64_t nt = (uint64_t)P * txns_per_rank;
        DV_LAUNCH(k_il_commits, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nt + kBlock - 1) / kBlock, 2048)),
                  kBlock, 0, s, m->verdict, xs, m->ilv);
        CHK(hip_fail2(hipGetLastError(), "k_il_commits"));
        vsend = m->ilv;
    }
    CHK(m->x->group(true));
    CHK(m->x->all_to_allv(reinterpret_cast<const uint8_t *>(m->send), sc.data(), sd.data(),
                          reinterpret_cast<uint8_t *>(m->recv), rc.data(), rd.data(), s));
    CHK(m->x->all_to_allv(vsend, tc.data(), td.data(), commit_out, uc.data(), ud.data(), s));
    CHK(m->x->group(false));

    // 6. epochs 0..P-1 on this partition's rows, in order (2PL: a written row
    //    has one committed txn, reads and writes in one launch; OCC / CALVIN:
    //    reads first)
    ctx_table0_cols(c, &f0, &pkey);
    // (xacc, the digest slots, zeroed by k_route_words)
    // (ordered lanes: after the previous group's execution, dv_lanes_order)
    CHK(lane_exec_begin(c, s));
    const bool fused = cfg.cc_alg == DV_NO_WAIT || cfg.cc_alg == DV_WAIT_DIE;
    const uint2 *recs = reinterpret_cast<const uint2 *>(m->recv);
    uint64_t off = 0;
    for (uint32_t e = 0; e < P; e++) {
        const uint64_t n = rcnt[e];
        if (n) {
            const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + kBlock - 1) / kBlock, 1024);
            if (fused) {
                DV_LAUNCH((k_route_exec<3>), blocks, kBlock, 0, s, recs + off, n, f0, pkey, m->xacc);
            } else {
                DV_LAUNCH((k_route_exec<1>), blocks, kBlock, 0, s, recs + off, n, f0, pkey, m->xacc);
                DV_LAUNCH((k_route_exec<2>), blocks, kBlock, 0, s, recs + off, n, f0, pkey, m->xacc);
            }
        }
        off += n;
    }
    CHK(hip_fail2(hipGetLastError(), "k_route_exec"));
    lane_exec_end(c, s);
    if (st) {
        *st = est;  // this rank's decision: rounds, sort passes, timings
        st->n_txn = n_txn64 * P;
        st->committed = committed;
        st->aborted = n_txn64 * P - committed;
    }
    if (defer && dfr) {  // the next group's vote reads the digest
        dfr->st = st;
        return DV_OK;
    }
    uint64_t slots[2 * kSlots];
    CHK(mail_get(m, s, reinterpret_cast<const uint64_t *>(m->xacc), 2 * kSlots, nullptr, 0, slots, nullptr));
    if (st) group_digest(st, slots);
    return DV_OK;
}
}  // namespace

extern "C" {

int dv_epoch_run_part(dv_ctx *c, const dv_epoch_dev *home, uint32_t txns_per_rank, uint8_t *d_commit,
                      dv_stats *st) {
    KProfScope kps_(c);
    const int r = run_part(c, home, nullptr, nullptr, false, txns_per_rank, d_commit, nullptr, st);
    if (r && c) lane_fail(c);  // (ordered lanes: the epochs after this one stop)
    return r;
}

int dv_epoch_group_run(dv_ctx *c, const dv_epoch_dev *homes, uint32_t n_homes, uint32_t txns_per_rank,
                       uint8_t *d_commit, dv_stats *st) {
    KProfScope kps_(c);
    const int r = run_group(c, homes, n_homes, txns_per_rank, d_commit, st);
    if (r && c) lane_fail(c);  // (ordered lanes waiting for this group's turn stop)
    return r;
}

int dv_epoch_group_run_batch(dv_ctx *c, const dv_epoch_dev *homes, uint32_t n_groups, uint32_t n_homes,
                             uint32_t txns_per_rank, uint8_t *const *d_commits, dv_stats *st) {
    KProfScope kps_(c);
    GroupDefer dfr;
    for (uint32_t g = 0; g < n_groups; g++) {
        const int r = run_group(c, homes ? homes + (size_t)g * n_homes : nullptr, n_homes, txns_per_rank,
                                d_commits ? d_commits[g] : nullptr, st ? st + g : nullptr, &dfr, g + 1 < n_groups);
        if (r) {  // (every rank of the communicator, at the same group)
            if (c) lane_fail(c);
            return r;
        }
    }
    return DV_OK;
}

int dv_comm_set_mode(dv_ctx *c, int mode) {
    const int flags = DV_COMM_WIDE_BATCHES | DV_COMM_POSITION_ORDER;
    if (!c || mode < 0 || (mode & ~flags) > 2) return DV_ERR_ARG;
    DvComm *m = ctx_comm(c);
    if (!m) return DV_ERR_STATE;
    m->mode = mode & ~flags;
    m->wide = (mode & DV_COMM_WIDE_BATCHES) != 0;
    m->position = (mode & DV_COMM_POSITION_ORDER) != 0;
    return DV_OK;
}

int dv_tpcc_epoch_run_part(dv_ctx *c, const dv_epoch_dev *home, const uint64_t *d_args, const uint8_t *d_owner,
                           uint32_t txns_per_rank, uint8_t *d_commit, uint64_t *d_oid, dv_stats *st) {
    KProfScope kps_(c);
    const int r = run_part(c, home, d_owner, d_args, true, txns_per_rank, d_commit, d_oid, st);
    if (r && c) lane_fail(c);  // (ordered lanes: the epochs after this one stop)
    return r;
}

}  // extern "C"
