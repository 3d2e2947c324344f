// dvcc_carry.hip -- abort carry-over into the next epoch.
//
// The reference retries an aborted txn: WorkerThread::abort (worker_thread.cpp:
// 160-172) hands its id to AbortQueue::enqueue, which holds it for a penalty
// and re-enqueues it as RTXN with its query unchanged (abort_queue.cpp:26-82).
// Here the penalty is one epoch: after an epoch is decided, the accesses of
// its aborted txns are compacted on the device, in sequence order and
// renumbered from 0, to open the next epoch ahead of the new txns -- they are
// older, so they keep their priority (WAIT_DIE keeps a restarted txn's
// timestamp).  Three launches: per-block counts, one scan of the block
// counts, then every carried txn copies its accesses.  A TPC-C epoch carries
// a fifth stream beside key, type, table and txn id: each access's 8-byte
// operation word (ARGS; the YCSB instantiations hold no trace of it).
#include "dvcc_common.h"

namespace dvcc {

constexpr uint32_t kCarryTpb = kBlock;  // txns per block: one per thread

__device__ __forceinline__ bool carried(const uint8_t *status, uint32_t t) {
    return status[t] != ST_COMMIT;  // aborted (nothing is undecided after the rounds)
}

// per block: aborted txns and their accesses
__global__ __launch_bounds__(kBlock) void k_carry_count(const uint8_t *__restrict__ status,
                                                        const uint32_t *__restrict__ tb_start,
                                                        const uint32_t *__restrict__ tb_end,
                                                        uint32_t n_txn, uint32_t *__restrict__ bt,
                                                        uint32_t *__restrict__ ba) {
    __shared__ uint32_t lds4[4];
    const uint32_t t = blockIdx.x * kCarryTpb + threadIdx.x;
    const bool cr = t < n_txn && carried(status, t);
    const uint32_t nt = cr ? 1u : 0u, na = cr ? tb_end[t] - tb_start[t] : 0u;
    uint32_t tt = 0, ta = 0;
    (void)block_excl_scan256(nt, lds4, &tt);
    (void)block_excl_scan256(na, lds4, &ta);
    if (threadIdx.x == 0) {
        bt[blockIdx.x] = tt;
        ba[blockIdx.x] = ta;
    }
}

// one block: exclusive scans of the block counts, in place
__global__ __launch_bounds__(kBlock) void k_carry_scan(uint32_t *__restrict__ bt, uint32_t *__restrict__ ba,
                                                       uint32_t nb) {
    __shared__ uint32_t lds4[4];
    const uint32_t per = (nb + kBlock - 1) / kBlock;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    constexpr uint32_t kR = 16;  // (nb <= 4,096 blocks, 1M txns: a thread's chunk in registers)
    if (per <= kR) {  // every load in flight at once (the loop waited out one round trip per entry: 10 us)
        uint32_t vt[kR], va[kR], st = 0, sa = 0;
#pragma unroll
        for (uint32_t k = 0; k < kR; k++) {
            const bool in = k < per && lo + k < nb;
            vt[k] = in ? bt[lo + k] : 0u;
            va[k] = in ? ba[lo + k] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kR; k++) {
            st += vt[k];
            sa += va[k];
        }
        uint32_t pt = block_excl_scan256(st, lds4, nullptr);
        uint32_t pa = block_excl_scan256(sa, lds4, nullptr);
#pragma unroll
        for (uint32_t k = 0; k < kR; k++) {
            if (k < per && lo + k < nb) {
                bt[lo + k] = pt;
                ba[lo + k] = pa;
            }
            pt += vt[k];
            pa += va[k];
        }
        return;
    }
    uint32_t st = 0, sa = 0;
    for (uint32_t i = lo; i < hi; i++) {
        st += bt[i];
        sa += ba[i];
    }
    uint32_t pt = block_excl_scan256(st, lds4, nullptr);
    uint32_t pa = block_excl_scan256(sa, lds4, nullptr);
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t vt = bt[i], va = ba[i];
        bt[i] = pt;
        ba[i] = pa;
        pt += vt;
        pa += va;
    }
}

// every carried txn with a new id below max_txn is copied; the last one
// reports the carried epoch's size (tot[0] txns, tot[1] accesses).
template <bool ARGS>
__global__ __launch_bounds__(kBlock) void k_carry_copy(
    const uint8_t *__restrict__ status, const uint32_t *__restrict__ tb_start,
    const uint32_t *__restrict__ tb_end, uint32_t n_txn, const uint32_t *__restrict__ bt,
    const uint32_t *__restrict__ ba, uint32_t max_txn, const uint64_t *__restrict__ keys,
    const uint8_t *__restrict__ types, const uint8_t *__restrict__ tables, uint64_t *__restrict__ okeys,
    uint8_t *__restrict__ otypes, uint32_t *__restrict__ otxn, uint8_t *__restrict__ otables,
    uint32_t *__restrict__ tot, const uint32_t *__restrict__ skip, const uint32_t *__restrict__ recs,
    uint32_t *__restrict__ orecs, uint32_t *__restrict__ otb, const uint64_t *__restrict__ args,
    uint64_t *__restrict__ oargs) {
    __shared__ uint32_t lds4[4];
    if (skip && *skip) return;  // (a refill behind a halted epoch: k_refill_plan)
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t t = blockIdx.x * kCarryTpb + threadIdx.x;
    const bool cr = t < n_txn && carried(status, t);
    const uint32_t a0 = cr ? tb_start[t] : 0u;
    uint32_t len = cr ? tb_end[t] - a0 : 0u;
    const uint32_t id = bt[blockIdx.x] + block_excl_scan256(cr ? 1u : 0u, lds4, nullptr);
    const uint32_t pos = ba[blockIdx.x] + block_excl_scan256(len, lds4, nullptr);
    const uint32_t total_txn = tot[2];  // carried txns before the cap (k_carry_total)
    const uint32_t last = total_txn < max_txn ? total_txn : max_txn;
    if (cr && id < max_txn && id + 1 == last) {
        tot[0] = last;
        tot[1] = pos + len;
    }
    if (!cr || id >= max_txn) len = 0;  // (ids grow with t: the cap cuts a suffix)
    else if (otb) otb[id] = pos;        // (tb form: the carried txn's boundary, dv_epoch_dev::txn_begin)
    // The block's txns hold one contiguous run of source accesses: the block
    // streams it (coalesced loads and stores), each access going to its txn's
    // destination plus its offset in the txn.  An access's txn: the last one
    // starting at or before it, by a binary search over the block's starts in
    // LDS -- made monotone by a suffix minimum, since an empty txn's range
    // (never written by the probe) may hold anything.  (An earlier form
    // spread each wave's carried accesses over its lanes by a shuffle search:
    // at a ~97 % carry rate that search, not the bytes, set its time.)
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    __shared__ uint32_t s_a0[kCarryTpb], s_id[kCarryTpb], s_sh[kCarryTpb], s_w[2][kCarryTpb / 64];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t a0s = t < n_txn ? tb_start[t] : 0u;
    const uint32_t src_len = t < n_txn ? tb_end[t] - a0s : 0u;
    uint32_t v = src_len ? a0s : kNone;  // suffix min of the non-empty txns' starts
    uint32_t e = src_len ? a0s + src_len : 0u;  // and the block's end of accesses (max)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_down(v, off, 64), oe = __shfl_down(e, off, 64);
        if (lane + (uint32_t)off < 64u) {
            v = o < v ? o : v;
            e = oe > e ? oe : e;
        }
    }
    if (lane == 0) {
        s_w[0][wave] = v;  // (lane 0: the wave's whole suffix)
        s_w[1][wave] = e;
    }
    __syncthreads();
    uint32_t hi = 0;
    for (uint32_t w = 0; w < kCarryTpb / 64; w++) {
        if (w > wave) v = s_w[0][w] < v ? s_w[0][w] : v;
        hi = s_w[1][w] > hi ? s_w[1][w] : hi;
    }
    s_a0[tid] = v;
    s_id[tid] = len ? id : kNone;
    s_sh[tid] = pos - a0;  // (mod 2^32: destination = source + shift)
    __syncthreads();
    const uint32_t lo = s_a0[0];
    for (uint32_t i = lo + tid; lo != kNone && i < hi; i += kCarryTpb) {
        uint32_t k = 0;
#pragma unroll
        for (uint32_t w = kCarryTpb / 2; w > 0; w >>= 1)
            if (s_a0[k + w] <= i) k += w;
        const uint32_t sid = s_id[k];
        if (sid == kNone) continue;
        const uint32_t o = i + s_sh[k];
        if (orecs) orecs[o] = recs[i];  // tb form: the 4-byte records (key | write << 31)
        if (!okeys) continue;
        okeys[o] = keys[i];
        otypes[o] = types[i];
        otxn[o] = sid;
        if (tables) otables[o] = tables[i];
        if (ARGS) oargs[o] = args[i];  // (TPC-C: the operation word, an 8-byte stream like the keys)
    }
}

// tot[2] = carried txns before the cap: the last block's exclusive prefix plus
// its own count; tot[0..1] cleared for k_carry_copy
__global__ void k_carry_total(const uint8_t *__restrict__ status, uint32_t n_txn, const uint32_t *bt,
                              uint32_t nb, uint32_t *tot) {
    uint32_t c = 0;
    for (uint32_t t = (nb - 1) * kCarryTpb + threadIdx.x; t < n_txn; t += blockDim.x)
        c += carried(status, t) ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (threadIdx.x == 0) {
        tot[0] = 0;
        tot[1] = 0;
        tot[2] = bt[nb - 1] + c;
    }
}

// ---- the closed loop on the device (dv_epoch_run_closed_loop): the next epoch is the
// carried txns (as above, capped at n_out), then fresh txns taken in order
// from a pool, starting at a device-side cursor that wraps around the pool.
// Nothing is read back: the epoch's access count stays on the device
// (dv_epoch_dev::n_acc_dev).  An epoch whose rounds halted has no final
// statuses yet: then every refill kernel is a no-op (the host redoes both).
// tot: [0] carried txns, [1] their accesses, [2] aborted before the cap,
// [3] the cursor's value, [4] skip (halted), [5] fresh txns (kRefillTot)
__device__ __forceinline__ bool refill_skip(const Counters *ctr) {
    return ctr && (ctr->halt || ctr->a_halt || input_err(ctr));  // (no ctr: the loop's first epoch)
}

__global__ void k_refill_plan(const uint8_t *__restrict__ status, uint32_t n_txn, const uint32_t *bt, uint32_t nb,
                              uint32_t *tot, uint32_t n_out, uint32_t *cursor, uint32_t pool_n,
                              const Counters *ctr) {
    uint32_t c = 0;
    for (uint32_t t = (nb ? nb - 1 : 0) * kCarryTpb + threadIdx.x; nb && t < n_txn; t += blockDim.x)
        c += carried(status, t) ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (threadIdx.x != 0) return;
    const uint32_t skip = refill_skip(ctr) ? 1u : 0u;
    const uint32_t total = nb ? bt[nb - 1] + c : 0u;
    const uint32_t C = total < n_out ? total : n_out;
    const uint32_t cur = *cursor, F = n_out - C;
    tot[0] = 0;
    tot[1] = 0;
    tot[2] = skip ? 0u : total;  // (skip: k_carry_copy copies nothing)
    tot[3] = cur;
    tot[4] = skip;
    tot[5] = F;
    if (!skip) *cursor = (uint32_t)(((uint64_t)cur + F) % pool_n);
}

// the fresh txns [cur, cur + F) of the pool (wrapping), renumbered after the
// C carried ones, their accesses after the carried accesses; the epoch's
// access count into *n_acc_dev
template <bool ARGS>
__global__ __launch_bounds__(kBlock) void k_refill_fresh(const uint64_t *__restrict__ keys,
                                                         const uint8_t *__restrict__ types,
                                                         const uint8_t *__restrict__ tables,
                                                         const uint32_t *__restrict__ txn,
                                                         const uint32_t *__restrict__ tb, uint32_t pool_n,
                                                         const uint32_t *__restrict__ tot, uint32_t n_out,
                                                         uint64_t *__restrict__ okeys, uint8_t *__restrict__ otypes,
                                                         uint32_t *__restrict__ otxn, uint8_t *__restrict__ otables,
                                                         uint32_t *__restrict__ n_acc_dev,
                                                         const uint32_t *__restrict__ precs,
                                                         uint32_t *__restrict__ orecs, uint32_t *__restrict__ otb,
                                                         const uint64_t *__restrict__ pargs,
                                                         uint64_t *__restrict__ oargs) {
    if (tot[4]) return;
    const uint32_t C = tot[2] < n_out ? tot[2] : n_out, A = tot[1], cur = tot[3], F = tot[5];
    const uint32_t e1 = cur + F < pool_n ? cur + F : pool_n;     // [cur, e1) then [0, F - (e1 - cur))
    const uint32_t n2 = F - (e1 - cur);
    const uint32_t b1 = tb[cur], fa1 = tb[e1] - b1, fa2 = tb[n2] - tb[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_acc_dev = A + fa1 + fa2;
    if (orecs) {  // tb form: the fresh txns' boundaries (and the epoch's end), then their records
        for (uint32_t f = blockIdx.x * kBlock + threadIdx.x; f <= F; f += gridDim.x * kBlock) {
            const uint32_t n1 = e1 - cur;
            otb[C + f] = A + (f <= n1 ? tb[cur + f] - b1 : fa1 + (tb[f - n1] - tb[0]));
        }
        for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < fa1 + fa2; i += gridDim.x * kBlock)
            orecs[A + i] = precs[i < fa1 ? b1 + i : tb[0] + (i - fa1)];
    }
    if (!okeys) return;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < fa1 + fa2; i += gridDim.x * kBlock) {
        const bool first = i < fa1;
        const uint32_t src = first ? b1 + i : tb[0] + (i - fa1);
        const uint32_t t = first ? txn[src] - cur : txn[src] + (pool_n - cur);
        okeys[A + i] = keys[src];
        otypes[A + i] = types[src];
        otxn[A + i] = C + t;
        if (otables) otables[A + i] = tables ? tables[src] : 0;
        if (ARGS) oargs[A + i] = pargs[src];
    }
}

// ---- the loop tracker (dv_closed_loop_track): identity through the refill.
// One 8-byte word per txn, src | born << 32.  k_track_carry runs behind
// k_refill_plan (bt[] and tot[] final).  A wave takes one 256-txn carry block,
// a lane four consecutive txns (32 contiguous bytes of identity words), so a
// txn's rank in its block is a wave scan -- no barrier on the way.  A carried
// txn's word moves to its new number, bt[b] plus that rank as in k_carry_copy;
// a committed txn's word goes to the commit log at the running count plus its
// rank among the epoch's commits, t - (carried before t) -- positions at or
// past log_cap are counted and not written.  Retries at commit, (k - born) /
// L, go into a histogram in LDS, flushed once per block with one atomic per
// non-empty bin, the block's counts with one atomic each -- not into the
// caller's arrays but into one of kTrackSlots copies (tr.part): every block of
// a 1M-txn epoch adding to the same 8-byte words took 126 us, 30 ns per block
// and address, one after the other.  k_track_fresh, the next launch, folds the
// copies into the histogram and the totals with plain stores and clears them.
// Every block reads *log_pos, so nobody in this launch writes it: one thread
// leaves the new count in the epoch's epoch_end slot and k_track_fresh copies
// it to *log_pos.
constexpr uint32_t kTrackPer = 4;  // txns per lane: a wave covers kCarryTpb
static_assert(kTrackPer * 64 == kCarryTpb, "a wave of k_track_carry takes one carry block");

__global__ __launch_bounds__(kBlock) void k_track_carry(const uint8_t *__restrict__ status, uint32_t n_txn,
                                                        const uint32_t *__restrict__ bt,
                                                        const uint32_t *__restrict__ tot, uint32_t n_out,
                                                        RefillTrack tr) {
    __shared__ uint32_t s_hist[kTrackBins];
    __shared__ uint32_t s_tot[4];  // committed, aborted, first aborts, most retries
    if (tot[4]) return;            // (a refill behind a halted epoch: k_refill_plan)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < tr.n_bins; i += kBlock) s_hist[i] = 0;
    if (tid < 4) s_tot[tid] = 0;
    __syncthreads();
    const uint32_t b = blockIdx.x * (kBlock / 64) + wave;  // the wave's carry block (past the last: idle)
    const uint64_t t0 = (uint64_t)b * kCarryTpb + lane * kTrackPer;
    const uint32_t nv = t0 >= n_txn ? 0u : (n_txn - t0 < kTrackPer ? (uint32_t)(n_txn - t0) : kTrackPer);
    uint64_t word[kTrackPer];
    bool cr[kTrackPer];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTrackPer; j++) {
        word[j] = j < nv ? tr.ids[t0 + j] : 0;
        cr[j] = j < nv && carried(status, (uint32_t)(t0 + j));
        c += cr[j] ? 1u : 0u;
    }
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += o;
    }
    // txns carried before this lane's first, in the whole epoch
    uint32_t r = ((uint64_t)b * kCarryTpb < n_txn ? bt[b] : 0u) + incl - c;
    const uint32_t pos0 = *tr.log_pos;
    uint32_t n_cm = 0, n_first = 0, mx = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTrackPer; j++) {
        if (j >= nv) continue;
        const uint32_t born = (uint32_t)(word[j] >> 32);
        if (cr[j]) {
            if (r < n_out) tr.oids[r] = word[j];
            r++;
            n_first += born == tr.k ? 1u : 0u;
            continue;
        }
        const uint64_t pos = (uint64_t)pos0 + ((uint32_t)(t0 + j) - r);
        if (pos < tr.log_cap) tr.log[pos] = word[j];
        const uint32_t retries = (tr.k - born) / tr.L;
        atomicAdd(&s_hist[retries < tr.n_bins - 1 ? retries : tr.n_bins - 1], 1u);
        mx = retries > mx ? retries : mx;
        n_cm++;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_cm += __shfl_xor(n_cm, off, 64);
        c += __shfl_xor(c, off, 64);
        n_first += __shfl_xor(n_first, off, 64);
        const uint32_t o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) {
        if (n_cm) atomicAdd(&s_tot[0], n_cm);
        if (c) atomicAdd(&s_tot[1], c);
        if (n_first) atomicAdd(&s_tot[2], n_first);
        if (mx) atomicMax(&s_tot[3], mx);
    }
    __syncthreads();
    uint32_t *const part = tr.part + (size_t)(blockIdx.x % kTrackSlots) * (tr.n_bins + 4);
    for (uint32_t i = tid; i < tr.n_bins; i += kBlock)
        if (s_hist[i]) atomicAdd(&part[i], s_hist[i]);
    if (tid < 3 && s_tot[tid]) atomicAdd(&part[tr.n_bins + tid], s_tot[tid]);
    if (tid == 3 && s_tot[3]) atomicMax(&part[tr.n_bins + 3], s_tot[3]);
    if (blockIdx.x == 0 && tid == 0) *tr.epoch_end = pos0 + (n_txn - tot[2]);
}

// what k_track_carry (or k_bo_park) left -- the commit count, and the
// kTrackSlots copies of the histogram and the counts, added to the caller's
// (one thread a word: plain 8-byte stores) and cleared for the next refill
__device__ __forceinline__ void track_fold(const RefillTrack &tr) {
    const uint32_t stride = tr.n_bins + 4;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < stride; i += gridDim.x * kBlock) {
        const bool is_max = i == tr.n_bins + 3;
        uint32_t v[kTrackSlots], sum = 0;
#pragma unroll
        for (uint32_t sl = 0; sl < kTrackSlots; sl++) v[sl] = tr.part[sl * stride + i];  // (all in flight)
#pragma unroll
        for (uint32_t sl = 0; sl < kTrackSlots; sl++) {
            sum = is_max ? (v[sl] > sum ? v[sl] : sum) : sum + v[sl];
            if (v[sl]) tr.part[sl * stride + i] = 0;
        }
        if (!sum) continue;
        uint64_t *const w = i < tr.n_bins ? &tr.hist[i] : &tr.totals[i - tr.n_bins];
        *w = is_max ? (*w > sum ? *w : (uint64_t)sum) : *w + sum;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *tr.log_pos = *tr.epoch_end;
}

// the F fresh txns' identity words behind the C carried ones: their pool index
// and the number of the epoch being built; and (prev: there was an epoch to
// log) the fold above
__global__ __launch_bounds__(kBlock) void k_track_fresh(const uint32_t *__restrict__ tot, uint32_t n_out,
                                                        uint32_t pool_n, int prev, RefillTrack tr) {
    if (tot[4]) return;
    const uint32_t C = tot[2] < n_out ? tot[2] : n_out, cur = tot[3], F = tot[5];
    for (uint32_t f = blockIdx.x * kBlock + threadIdx.x; f < F && C + f < n_out; f += gridDim.x * kBlock)
        tr.oids[C + f] = (((uint64_t)cur + f) % pool_n) | (uint64_t)tr.k_next << 32;
    if (prev) track_fold(tr);
}

static void launch_refill_backoff(hipStream_t s, const RefillReq &q);

void launch_refill(hipStream_t s, const RefillReq &q) {
    if (q.bo) return launch_refill_backoff(s, q);
    const DecidedEpoch &e = q.ep;
    const AccessCols &in = q.in, &p = q.pool.cols;
    const AccessOut &o = q.out;
    uint32_t *const bt = q.ws.bt, *const ba = q.ws.ba, *const tot = q.ws.tot;
    const uint32_t nb = carry_blocks(e.n_txn);
    if (nb) {
        DV_LAUNCH(k_carry_count, nb, kBlock, 0, s, e.status, e.tb_start, e.tb_end, e.n_txn, bt, ba);
        DV_LAUNCH(k_carry_scan, 1, kBlock, 0, s, bt, ba, nb);
    }
    DV_LAUNCH(k_refill_plan, 1, 64, 0, s, e.status, e.n_txn, bt, nb, tot, q.n_out, q.pool.cursor, q.pool.n, e.ctr);
    const uint32_t *skip = tot + 4;
    const uint64_t *no_args = nullptr;
    if (nb && o.args)
        DV_LAUNCH((k_carry_copy<true>), nb, kBlock, 0, s, e.status, e.tb_start, e.tb_end, e.n_txn, bt, ba, q.n_out,
                  in.keys, in.types, in.tables, o.keys, o.types, o.txn, o.tables, tot, skip, in.recs, o.recs, o.tb,
                  in.args, o.args);
    else if (nb)
        DV_LAUNCH((k_carry_copy<false>), nb, kBlock, 0, s, e.status, e.tb_start, e.tb_end, e.n_txn, bt, ba, q.n_out,
                  in.keys, in.types, in.tables, o.keys, o.types, o.txn, o.tables, tot, skip, in.recs, o.recs, o.tb,
                  no_args, o.args);
    const uint64_t g = (q.acc_bound + kBlock - 1) / kBlock;
    const uint32_t grid = (uint32_t)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
    if (o.args)
        DV_LAUNCH((k_refill_fresh<true>), grid, kBlock, 0, s, p.keys, p.types, p.tables, p.txn, q.pool.tb, q.pool.n,
                  tot, q.n_out, o.keys, o.types, o.txn, o.tables, o.n_acc_dev, p.recs, o.recs, o.tb, p.args, o.args);
    else
        DV_LAUNCH((k_refill_fresh<false>), grid, kBlock, 0, s, p.keys, p.types, p.tables, p.txn, q.pool.tb, q.pool.n,
                  tot, q.n_out, o.keys, o.types, o.txn, o.tables, o.n_acc_dev, p.recs, o.recs, o.tb, no_args, o.args);
    if (!q.trk) return;
    constexpr uint32_t wpb = kBlock / 64;  // (k_track_carry: a wave per carry block)
    if (nb)
        DV_LAUNCH(k_track_carry, (nb + wpb - 1) / wpb, kBlock, 0, s, e.status, e.n_txn, bt, tot, q.n_out, *q.trk);
    const uint32_t gf = (q.n_out + kBlock - 1) / kBlock;
    DV_LAUNCH(k_track_fresh, gf < 1 ? 1 : (gf > 1024 ? 1024 : gf), kBlock, 0, s, tot, q.n_out, q.pool.n, nb ? 1 : 0,
              *q.trk);
}

// ---- back-off (dv_closed_loop_backoff): the reference's AbortQueue::enqueue
// meant penalty * 2^abort_cnt capped at a maximum (abort_queue.cpp:26-31;
// written with ^ as XOR and max for min).  Here the penalty is
// counted in epochs: a txn's a-th abort parks it min(2^(a-1), D) epochs ahead
// in a ring of D slots, slot e % D holding what falls due in epoch e.  A
// parked txn is its identity word and an abort count byte (9 bytes); its
// accesses are read from the pool again when it is released.  The chain behind
// epoch k (building epoch e = k + 1, all kernel boundaries, no flags; under L
// decision lanes -- dv_closed_loop_backoff_lanes -- e = k + L, on epoch k's
// lane, and the park's delays count from e - 1, so the a-th abort costs
// L - 1 + min(2^(a-1), D) epochs; the chain is the same):
//   k_bo_count   per 256-txn carry block and delay class, the aborts
//   k_bo_scan    a workgroup per class: exclusive scan over the blocks
//   k_bo_plan    one thread: the skip word; per class its slot and the slot's
//                count before (the scatter's base), the counts after; the
//                release R = min(count[e % D], n_out), the spill behind it
//                (to the tail of slot (e + 1) % D), F = n_out - R, the cursor
//   k_bo_park    the scatter (base + block prefix + rank within the class, in
//                sequence order) and the tracker's pass over the commits
//   k_bo_spill   the spill's words and bytes to the next slot's tail
//   k_bo_gather_count / k_bo_scan / k_bo_gather_copy   the new epoch: src from
//                the slot (j < R) or the cursor range, length from pool_begin,
//                the accesses streamed from the pool
//   k_bo_fold    the tracker's fold (track_fold) and the wait sum
// Positions at or past the slots' capacity are counted (lost) and not written.
// bw[]: the plan words
enum : uint32_t {
    BW_CTOT = 0,    // [kBoClasses] aborts per class
    BW_BASE = 5,    // [kBoClasses] the class's slot count before the park
    BW_SLOT = 10,   // [kBoClasses] the class's slot
    BW_SRC = 15,    // the slot released
    BW_DST = 16,    // the slot taking the spill
    BW_TAIL = 17,   // ... its count before the spill
    BW_SPILL = 18,  // spill entries written
    BW_GTOT = 19,   // the new epoch's accesses
};
static_assert(BW_GTOT < kBoWords, "plan words");

// the delay class of an abort whose txn had aborted `ab` times before:
// delay min(2^ab, D)
__device__ __forceinline__ uint32_t bo_class(uint32_t ab, uint32_t lgD) { return ab < lgD ? ab : lgD; }

__global__ __launch_bounds__(kBlock) void k_bo_count(const uint8_t *__restrict__ status,
                                                     const uint8_t *__restrict__ aborts, uint32_t n_txn,
                                                     uint32_t nb, uint32_t lgD, uint32_t *__restrict__ cls) {
    __shared__ uint32_t s_c[kBoClasses];
    if (threadIdx.x < kBoClasses) s_c[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t t = blockIdx.x * kCarryTpb + threadIdx.x;
    const bool cr = t < n_txn && carried(status, t);
    const uint32_t ci = cr ? bo_class(aborts[t], lgD) : kBoClasses;
#pragma unroll
    for (uint32_t c = 0; c < kBoClasses; c++) {
        const uint64_t m = __ballot(ci == c);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_c[c], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x <= lgD) cls[threadIdx.x * nb + blockIdx.x] = s_c[threadIdx.x];
}

// workgroup r: exclusive scan of row r of c (n words a row) in place, the
// row's total into totals[r] (n <= 4,096: a thread's chunk in registers, as
// k_carry_scan)
__global__ __launch_bounds__(kBlock) void k_bo_scan(uint32_t *__restrict__ c, uint32_t n,
                                                    uint32_t *__restrict__ totals) {
    __shared__ uint32_t lds4[4];
    uint32_t *const row = c + (size_t)blockIdx.x * n;
    const uint32_t per = (n + kBlock - 1) / kBlock;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    constexpr uint32_t kR = 16;
    uint32_t tot = 0;
    if (per <= kR) {
        uint32_t v[kR], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kR; k++) v[k] = k < per && lo + k < n ? row[lo + k] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kR; k++) sum += v[k];
        uint32_t pre = block_excl_scan256(sum, lds4, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kR; k++) {
            if (k < per && lo + k < n) row[lo + k] = pre;
            pre += v[k];
        }
    } else {
        uint32_t sum = 0;
        for (uint32_t i = lo; i < hi; i++) sum += row[i];
        uint32_t pre = block_excl_scan256(sum, lds4, &tot);
        for (uint32_t i = lo; i < hi; i++) {
            const uint32_t x = row[i];
            row[i] = pre;
            pre += x;
        }
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = tot;
}

// e: the epoch being built; the ring's clock for the park before it is e - 1
// (prev: an epoch was decided -- epoch e - L under L decision lanes, whose
// aborts cannot return before e: the delays count from e - 1, and for one
// lane e - 1 is the epoch decided)
__global__ void k_bo_plan(int prev, uint32_t e, uint32_t n_out, uint32_t *cursor, uint32_t pool_n,
                          const Counters *ctr, uint32_t *tot, RefillBackoff bo) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t skip = prev && refill_skip(ctr) ? 1u : 0u;
    tot[4] = skip;
    if (skip) return;
    const uint32_t mask = bo.D - 1;
    uint32_t aborted = 0;
    uint64_t lost = 0;
    for (uint32_t c = 0; prev && c <= bo.lgD; c++) {  // (the delays 1 .. D fall into distinct slots)
        const uint32_t slot = (e - 1u + (1u << c)) & mask, n = bo.bw[BW_CTOT + c];
        const uint32_t base = bo.slot_count[slot] < bo.cap ? bo.slot_count[slot] : bo.cap;
        const uint64_t want = (uint64_t)base + n;
        const uint32_t now = want < bo.cap ? (uint32_t)want : bo.cap;
        bo.bw[BW_BASE + c] = base;
        bo.bw[BW_SLOT + c] = slot;
        bo.slot_count[slot] = now;
        lost += want - now;
        aborted += n;
    }
    const uint32_t s = e & mask, s2 = (e + 1) & mask;
    const uint32_t cnt = bo.slot_count[s] < bo.cap ? bo.slot_count[s] : bo.cap;
    const uint32_t R = cnt < n_out ? cnt : n_out, sp = cnt - R;
    uint32_t tail = 0, moved = 0;
    bo.slot_count[s] = 0;
    if (s2 != s) {
        tail = bo.slot_count[s2] < bo.cap ? bo.slot_count[s2] : bo.cap;
        moved = sp < bo.cap - tail ? sp : bo.cap - tail;
        bo.slot_count[s2] = tail + moved;
    }
    lost += sp - moved;  // (D = 1 never spills: at most n_out txns abort)
    const uint32_t F = n_out - R, cur = *cursor;
    *cursor = (uint32_t)(((uint64_t)cur + F) % pool_n);
    bo.bw[BW_SRC] = s;
    bo.bw[BW_DST] = s2;
    bo.bw[BW_TAIL] = tail;
    bo.bw[BW_SPILL] = moved;
    tot[0] = R;
    tot[1] = sp;
    tot[2] = aborted;
    tot[3] = cur;
    tot[5] = F;
    uint64_t parked = 0;
    for (uint32_t i = 0; i < bo.D; i++) parked += bo.slot_count[i];
    bo.counters[0] += sp;
    bo.counters[1] += lost;
    bo.counters[3] = parked;
    *bo.lost += lost;
}

// k_track_carry's pass with the ring in place of the next epoch: a wave takes
// one 256-txn carry block, a lane four consecutive txns.  An aborted txn goes
// to its class's slot at the slot's count before (bw) + the aborts of its
// class in the blocks before (cls) + its rank in its class in the block -- a
// wave scan of the lanes' class counts, ten bits a class, three classes to a
// word.  A committed txn is logged as k_track_carry logs it; the histogram
// bins it by its abort count, and (k - born), the epochs it took, is summed
// into one of kTrackSlots 8-byte copies (k_bo_fold adds them up).
__global__ __launch_bounds__(kBlock) void k_bo_park(const uint8_t *__restrict__ status, uint32_t n_txn,
                                                    uint32_t nb, const uint32_t *__restrict__ tot, RefillTrack tr,
                                                    RefillBackoff bo) {
    __shared__ uint32_t s_hist[kTrackBins];
    __shared__ uint32_t s_tot[4];  // committed, aborted, first aborts, most aborts at a commit
    __shared__ unsigned long long s_wait;
    if (tot[4]) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < tr.n_bins; i += kBlock) s_hist[i] = 0;
    if (tid < 4) s_tot[tid] = 0;
    if (tid == 0) s_wait = 0;
    __syncthreads();
    const uint32_t b = blockIdx.x * (kBlock / 64) + wave;  // the wave's carry block (past the last: idle)
    const bool live = b < nb;
    const uint64_t t0 = (uint64_t)b * kCarryTpb + lane * kTrackPer;
    const uint32_t nv = !live || t0 >= n_txn ? 0u : (n_txn - t0 < kTrackPer ? (uint32_t)(n_txn - t0) : kTrackPer);
    uint64_t word[kTrackPer];
    uint32_t ab[kTrackPer];
    bool cr[kTrackPer];
    uint32_t c = 0, c012 = 0, c34 = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTrackPer; j++) {
        word[j] = j < nv ? tr.ids[t0 + j] : 0;
        ab[j] = j < nv ? bo.aborts[t0 + j] : 0u;
        cr[j] = j < nv && carried(status, (uint32_t)(t0 + j));
        if (!cr[j]) continue;
        const uint32_t ci = bo_class(ab[j], bo.lgD);
        c++;
        if (ci < 3) c012 += 1u << (10 * ci);
        else c34 += 1u << (10 * (ci - 3));
    }
    const uint32_t r012 = wave_incl_sum(c012, lane) - c012, r34 = wave_incl_sum(c34, lane) - c34;
    // per class: where the block's aborts of that class start in their slot
    uint32_t at[kBoClasses], rank[kBoClasses], before = 0;
#pragma unroll
    for (uint32_t ci = 0; ci < kBoClasses; ci++) {
        const uint32_t pre = live && ci <= bo.lgD ? bo.cls[ci * nb + b] : 0u;
        at[ci] = ci <= bo.lgD ? bo.bw[BW_BASE + ci] + pre : 0u;
        rank[ci] = ((ci < 3 ? r012 >> (10 * (ci % 3)) : r34 >> (10 * (ci % 3))) & 1023u);
        before += pre;
    }
    uint32_t r = before + wave_incl_sum(c, lane) - c;  // txns aborted before this lane's first, in the whole epoch
    const uint32_t pos0 = *tr.log_pos;
    uint32_t n_cm = 0, n_first = 0, mx = 0;
    unsigned long long wait = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTrackPer; j++) {
        if (j >= nv) continue;
        const uint32_t born = (uint32_t)(word[j] >> 32);
        if (cr[j]) {
            const uint32_t ci = bo_class(ab[j], bo.lgD);
            uint32_t p = 0, slot = 0;
#pragma unroll
            for (uint32_t q = 0; q < kBoClasses; q++)
                if (q == ci) {
                    p = at[q] + rank[q];
                    rank[q]++;
                    slot = bo.bw[BW_SLOT + q];
                }
            if (p < bo.cap) {
                bo.park_ids[(size_t)slot * bo.cap + p] = word[j];
                bo.park_aborts[(size_t)slot * bo.cap + p] = (uint8_t)(ab[j] < 255 ? ab[j] + 1 : 255);
            }
            r++;
            n_first += ab[j] == 0 ? 1u : 0u;
            continue;
        }
        const uint64_t pos = (uint64_t)pos0 + ((uint32_t)(t0 + j) - r);
        if (pos < tr.log_cap) tr.log[pos] = word[j];
        atomicAdd(&s_hist[ab[j] < tr.n_bins - 1 ? ab[j] : tr.n_bins - 1], 1u);
        mx = ab[j] > mx ? ab[j] : mx;
        wait += tr.k - born;
        n_cm++;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_cm += __shfl_xor(n_cm, off, 64);
        c += __shfl_xor(c, off, 64);
        n_first += __shfl_xor(n_first, off, 64);
        const uint32_t o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
        wait += __shfl_xor(wait, off, 64);
    }
    if (lane == 0) {
        if (n_cm) atomicAdd(&s_tot[0], n_cm);
        if (c) atomicAdd(&s_tot[1], c);
        if (n_first) atomicAdd(&s_tot[2], n_first);
        if (mx) atomicMax(&s_tot[3], mx);
        if (wait) atomicAdd(&s_wait, wait);
    }
    __syncthreads();
    uint32_t *const part = tr.part + (size_t)(blockIdx.x % kTrackSlots) * (tr.n_bins + 4);
    for (uint32_t i = tid; i < tr.n_bins; i += kBlock)
        if (s_hist[i]) atomicAdd(&part[i], s_hist[i]);
    if (tid < 3 && s_tot[tid]) atomicAdd(&part[tr.n_bins + tid], s_tot[tid]);
    if (tid == 3 && s_tot[3]) atomicMax(&part[tr.n_bins + 3], s_tot[3]);
    if (tid == 4 && s_wait) atomicAdd(&bo.wpart[blockIdx.x % kTrackSlots], s_wait);
    if (blockIdx.x == 0 && tid == 0) *tr.epoch_end = pos0 + (n_txn - tot[2]);
}

// the released slot's entries behind the first R, to the next slot's tail
__global__ __launch_bounds__(kBlock) void k_bo_spill(const uint32_t *__restrict__ tot, RefillBackoff bo) {
    if (tot[4]) return;
    const uint32_t n = bo.bw[BW_SPILL];
    const size_t from = (size_t)bo.bw[BW_SRC] * bo.cap + tot[0], to = (size_t)bo.bw[BW_DST] * bo.cap + bo.bw[BW_TAIL];
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        bo.park_ids[to + i] = bo.park_ids[from + i];
        bo.park_aborts[to + i] = bo.park_aborts[from + i];
    }
}

// the new epoch's txn j: the released slot's j-th entry, or the (j - R)-th
// fresh pool txn; its identity word and abort count, and per block the
// accesses (a src outside the pool -- a ring the caller filled -- has none)
__global__ __launch_bounds__(kBlock) void k_bo_gather_count(const uint32_t *__restrict__ tot, uint32_t n_out,
                                                            const uint32_t *__restrict__ ptb, uint32_t pool_n,
                                                            uint64_t *__restrict__ oids, uint32_t k_next,
                                                            RefillBackoff bo) {
    __shared__ uint32_t lds4[4];
    if (tot[4]) return;
    const uint32_t j = blockIdx.x * kCarryTpb + threadIdx.x, R = tot[0], cur = tot[3];
    uint32_t len = 0;
    if (j < n_out) {
        uint64_t w;
        uint8_t a = 0;
        if (j < R) {
            const size_t p = (size_t)bo.bw[BW_SRC] * bo.cap + j;
            w = bo.park_ids[p];
            a = bo.park_aborts[p];
        } else {
            w = (((uint64_t)cur + (j - R)) % pool_n) | (uint64_t)k_next << 32;
        }
        const uint32_t src = (uint32_t)w;
        len = src < pool_n ? ptb[src + 1] - ptb[src] : 0u;
        oids[j] = w;
        bo.oaborts[j] = a;
    }
    uint32_t total = 0;
    (void)block_excl_scan256(len, lds4, &total);
    if (threadIdx.x == 0) bo.gb[blockIdx.x] = total;
}

// every txn's boundary, then the block streams its txns' accesses from the
// pool: an access's txn by a binary search over the block's output starts in
// LDS (non-decreasing: an exclusive scan), as k_carry_copy.  ARGS (the TPC-C
// loop): an access's operation word comes with it, as in k_carry_copy and
// k_refill_fresh -- one more 8-byte gather from the same contiguous run of the
// txn, one more coalesced store
template <bool ARGS>
__global__ __launch_bounds__(kBlock) void k_bo_gather_copy(
    const uint32_t *__restrict__ tot, uint32_t n_out, const uint64_t *__restrict__ oids,
    const uint64_t *__restrict__ pkeys, const uint8_t *__restrict__ ptypes, const uint8_t *__restrict__ ptables,
    const uint32_t *__restrict__ ptb, uint32_t pool_n, const uint32_t *__restrict__ precs,
    uint64_t *__restrict__ okeys, uint8_t *__restrict__ otypes, uint32_t *__restrict__ otxn,
    uint8_t *__restrict__ otables, uint32_t *__restrict__ orecs, uint32_t *__restrict__ otb,
    uint32_t *__restrict__ n_acc_dev, uint64_t acc_cap, RefillBackoff bo, const uint64_t *__restrict__ pargs,
    uint64_t *__restrict__ oargs) {
    __shared__ uint32_t lds4[4];
    __shared__ uint32_t s_st[kCarryTpb], s_p0[kCarryTpb];
    if (tot[4]) return;
    const uint32_t tid = threadIdx.x, j = blockIdx.x * kCarryTpb + tid;
    uint32_t p0 = 0, len = 0;
    if (j < n_out) {
        const uint32_t src = (uint32_t)oids[j];
        if (src < pool_n) {
            p0 = ptb[src];
            len = ptb[src + 1] - p0;
        }
    }
    uint32_t btot = 0;
    const uint32_t st = block_excl_scan256(len, lds4, &btot), base = bo.gb[blockIdx.x];
    if (j < n_out && otb) otb[j] = base + st;
    if (blockIdx.x == 0 && tid == 0) {
        *n_acc_dev = bo.bw[BW_GTOT];
        if (otb) otb[n_out] = bo.bw[BW_GTOT];  // (the closing boundary)
    }
    s_st[tid] = st;  // (a thread past n_out: btot, above every access)
    s_p0[tid] = p0;
    __syncthreads();
    for (uint32_t i = tid; i < btot; i += kCarryTpb) {
        uint32_t q = 0;
#pragma unroll
        for (uint32_t w = kCarryTpb / 2; w > 0; w >>= 1)
            if (s_st[q + w] <= i) q += w;
        const uint32_t a = s_p0[q] + (i - s_st[q]), o = base + i;
        if (o >= acc_cap) continue;  // (a pool txn longer than the pool's max_txn_acc: nothing past the buffers)
        if (orecs) orecs[o] = precs[a];
        if (!okeys) continue;
        okeys[o] = pkeys[a];
        otypes[o] = ptypes[a];
        otxn[o] = blockIdx.x * kCarryTpb + q;
        if (otables) otables[o] = ptables ? ptables[a] : 0;
        if (ARGS) oargs[o] = pargs[a];
    }
}

__global__ __launch_bounds__(kBlock) void k_bo_fold(const uint32_t *__restrict__ tot, RefillTrack tr,
                                                    RefillBackoff bo) {
    if (tot[4]) return;
    track_fold(tr);
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    unsigned long long v[kTrackSlots], sum = 0;
#pragma unroll
    for (uint32_t sl = 0; sl < kTrackSlots; sl++) v[sl] = bo.wpart[sl];
#pragma unroll
    for (uint32_t sl = 0; sl < kTrackSlots; sl++) {
        sum += v[sl];
        if (v[sl]) bo.wpart[sl] = 0;
    }
    if (sum) bo.counters[2] += sum;
}

static void launch_refill_backoff(hipStream_t s, const RefillReq &q) {
    const RefillTrack &trk = *q.trk;
    const RefillBackoff &bo = *q.bo;
    const AccessCols &p = q.pool.cols;
    const AccessOut &o = q.out;
    const uint32_t n_txn = q.ep.n_txn, n_out = q.n_out, pool_n = q.pool.n;
    uint32_t *const tot = q.ws.tot;
    const uint32_t nb = carry_blocks(n_txn), nbo = carry_blocks(n_out);
    constexpr uint32_t wpb = kBlock / 64;  // (k_bo_park: a wave per carry block)
    if (nb) {
        DV_LAUNCH(k_bo_count, nb, kBlock, 0, s, q.ep.status, bo.aborts, n_txn, nb, bo.lgD, bo.cls);
        DV_LAUNCH(k_bo_scan, bo.lgD + 1, kBlock, 0, s, bo.cls, nb, bo.bw + BW_CTOT);
    }
    DV_LAUNCH(k_bo_plan, 1, 64, 0, s, nb ? 1 : 0, trk.k_next, n_out, q.pool.cursor, pool_n, q.ep.ctr, tot, bo);
    if (nb) DV_LAUNCH(k_bo_park, (nb + wpb - 1) / wpb, kBlock, 0, s, q.ep.status, n_txn, nb, tot, trk, bo);
    const uint32_t gs = (bo.cap + kBlock - 1) / kBlock;
    DV_LAUNCH(k_bo_spill, gs < 1 ? 1 : (gs > 1024 ? 1024 : gs), kBlock, 0, s, tot, bo);
    DV_LAUNCH(k_bo_gather_count, nbo, kBlock, 0, s, tot, n_out, q.pool.tb, pool_n, trk.oids, trk.k_next, bo);
    DV_LAUNCH(k_bo_scan, 1, kBlock, 0, s, bo.gb, nbo, bo.bw + BW_GTOT);
    const uint64_t *no_args = nullptr;
    if (o.args)
        DV_LAUNCH((k_bo_gather_copy<true>), nbo, kBlock, 0, s, tot, n_out, trk.oids, p.keys, p.types, p.tables,
                  q.pool.tb, pool_n, p.recs, o.keys, o.types, o.txn, o.tables, o.recs, o.tb, o.n_acc_dev, q.acc_bound,
                  bo, p.args, o.args);
    else
        DV_LAUNCH((k_bo_gather_copy<false>), nbo, kBlock, 0, s, tot, n_out, trk.oids, p.keys, p.types, p.tables,
                  q.pool.tb, pool_n, p.recs, o.keys, o.types, o.txn, o.tables, o.recs, o.tb, o.n_acc_dev, q.acc_bound,
                  bo, no_args, o.args);
    if (nb) {
        const uint32_t gf = (trk.n_bins + 4 + kBlock - 1) / kBlock;
        DV_LAUNCH(k_bo_fold, gf, kBlock, 0, s, tot, trk, bo);
    }
}

// a client batch's per-txn access ranges from its acc_txn (non-decreasing;
// ids at or past n_txn were rejected by the run that decided it): zeroed
// first (a txn without accesses keeps an empty range), then each run's ends
__global__ void k_txn_ranges_zero(uint32_t *__restrict__ tbs, uint32_t *__restrict__ tbe, uint32_t n_txn) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_txn; t += gridDim.x * blockDim.x)
        tbs[t] = tbe[t] = 0;
}
__global__ void k_txn_ranges(const uint32_t *__restrict__ acc_txn, uint64_t n, uint32_t n_txn,
                             uint32_t *__restrict__ tbs, uint32_t *__restrict__ tbe) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t t = acc_txn[i];
        if (t >= n_txn) continue;
        if (i == 0 || acc_txn[i - 1] != t) tbs[t] = (uint32_t)i;
        if (i + 1 == n || acc_txn[i + 1] != t) tbe[t] = (uint32_t)(i + 1);
    }
}

void launch_txn_ranges(hipStream_t s, const uint32_t *acc_txn, uint64_t n, uint32_t n_txn, uint32_t *tbs,
                       uint32_t *tbe) {
    if (!n_txn) return;
    const uint32_t gt = (n_txn + kBlock - 1) / kBlock;
    DV_LAUNCH(k_txn_ranges_zero, gt < 2048 ? gt : 2048, kBlock, 0, s, tbs, tbe, n_txn);
    if (!n) return;
    const uint64_t ga = (n + kBlock - 1) / kBlock;
    DV_LAUNCH(k_txn_ranges, (uint32_t)(ga < 4096 ? ga : 4096), kBlock, 0, s, acc_txn, n, n_txn, tbs, tbe);
}

uint32_t carry_blocks(uint32_t n_txn) { return n_txn ? (n_txn + kCarryTpb - 1) / kCarryTpb : 0; }

void launch_carry(hipStream_t s, const CarryReq &q) {
    const DecidedEpoch &e = q.ep;
    const AccessCols &in = q.in;
    const AccessOut &o = q.out;
    uint32_t *const bt = q.ws.bt, *const ba = q.ws.ba, *const tot = q.ws.tot;
    const uint32_t nb = carry_blocks(e.n_txn);
    if (!nb) {
        (void)hipMemsetAsync(tot, 0, 3 * sizeof(uint32_t), s);
        return;
    }
    DV_LAUNCH(k_carry_count, nb, kBlock, 0, s, e.status, e.tb_start, e.tb_end, e.n_txn, bt, ba);
    DV_LAUNCH(k_carry_scan, 1, kBlock, 0, s, bt, ba, nb);
    DV_LAUNCH(k_carry_total, 1, 64, 0, s, e.status, e.n_txn, bt, nb, tot);
    const uint32_t *none = nullptr;
    uint32_t *onone = nullptr;
    if (o.args)
        DV_LAUNCH((k_carry_copy<true>), nb, kBlock, 0, s, e.status, e.tb_start, e.tb_end, e.n_txn, bt, ba, q.max_txn,
                  in.keys, in.types, in.tables, o.keys, o.types, o.txn, o.tables, tot, none, none, onone, onone,
                  in.args, o.args);
    else
        DV_LAUNCH((k_carry_copy<false>), nb, kBlock, 0, s, e.status, e.tb_start, e.tb_end, e.n_txn, bt, ba, q.max_txn,
                  in.keys, in.types, in.tables, o.keys, o.types, o.txn, o.tables, tot, none, none, onone, onone,
                  in.args, o.args);
}

}  // namespace dvcc
