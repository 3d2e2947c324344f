// dvcc_wire.hip -- Deneva client batches decoded on the device.
//
// What csrc/wire.cpp does message by message on one core (dv_wire_open's
// checks, dv_wire_decode's arrays) for a receive queue's bytes already in
// device memory, taken into a device-resident epoch (include/dvcc.h,
// dv_wire_ingest_device*).  A batch is at most 4,096 bytes and a short chain of
// variable-length messages, so a wave takes one: its bytes staged in LDS,
// the chain walked once (at most 48 links), then every partition and request
// checked or scattered by all lanes.  Four entries, four launches each:
//   k_wire_check*  per batch {txns, accesses, longest txn}, the message
//                  offsets, and the first malformed batch
//   k_wire_scan*   per chunk of kWireChunk batches: prefixes inside the chunk
//   k_wire_plan*   one workgroup: the chunks' prefixes, the first batch that
//                  does not fit, the result record, the closing boundary
//   k_wire_emit*   the taken batches' boundaries, reply fields and accesses
// YCSB CL_QRY batches (dv_wire_ingest_device) are taken whole.  TPC-C CL_QRY
// batches (dv_wire_ingest_device_tpcc) take the same scan and plan between
// k_wire_check_tpcc and k_wire_emit_tpcc, which expand every message to its
// access list as dv_tpcc_expand does.  CALVIN sequencer streams
// (dv_wire_ingest_device_calvin, YCSB; k_wire_*_calvin) have a header that
// carries batch_id, RDONE ends a batch, and the epoch is cut at a message;
// TPC-C under CALVIN (dv_wire_ingest_device_calvin_tpcc) is the two composed,
// k_wire_check_calvin_tpcc and k_wire_emit_calvin_tpcc around the stream's
// scan and plan.  What the dialects share is written once, in the helpers of
// the unnamed namespaces below: the staging prologues, the chain walk, the
// partition and request loops, the txn fields, the plan's capacity cut, the
// TPC-C field checks and expansion, the run of an mbuf.  A dialect is a
// compile-time parameter (Client, Calvin), never a switch inside a kernel; a
// helper with a barrier is reached by every wave of its block, live or not.
// And, for the replies, the committed txns' fields compacted in txn order
// (k_reply_count / k_reply_scan / k_reply_emit, like the carry-over's).
// The byte stream has no alignment (COPY_BUF): fields are assembled from the
// aligned words of the LDS image, never dereferenced in place.
#include "dvcc_common.h"

namespace dvcc {

namespace {

constexpr uint32_t kWireMsgMax = DV_WIRE_MSG_MAX;
// a batch's LDS image: its bytes from the 16-byte line its first byte lies
// in (up to 15 bytes in front) to the line of its last, and one line more so
// a field's last word may be read past it
constexpr uint32_t kStageQ = (kWireMsgMax + 15 + 15) / 16 + 1;
constexpr uint32_t kReqBytes = 24;     // sizeof(ycsb_request)
constexpr uint32_t kReqMax = 128;      // the engine's longest txn (kMaxPos)
constexpr uint32_t kNoBatch = 0xFFFFFFFFu;
constexpr uint32_t kCalTxnId = 4, kCalBatchId = 12;  // CALVIN header offsets
constexpr uint64_t kNoBatchId = ~0ull;

// A dialect's message (Message::mget_size): kHdr bytes of rtype, txn_id,
// [batch_id,] mq_time, 7 latencies; a CL_QRY goes on to kFixed with
// client_startts and the partition count.  kStride: messages a batch may hold,
// the stride of WireWs::moff.  kRdone: an RDONE, the header alone, is a message.
struct Client {
    static constexpr uint32_t kHdr = 76, kFixed = 92, kStride = kWireMaxMsg;
    static constexpr bool kRdone = false;
};
struct Calvin {
    static constexpr uint32_t kHdr = 84, kFixed = 100, kStride = kWireCalvinMaxMsg;
    static constexpr bool kRdone = true;
};

struct Stage {
    const uint32_t *w;  // the image's words
    uint32_t sh;        // the batch's first byte in it
    __device__ __forceinline__ uint32_t u32(uint32_t o) const {
        const uint32_t a = sh + o, i = a >> 2;
        return (uint32_t)((((uint64_t)w[i + 1] << 32) | w[i]) >> ((a & 3u) * 8u));
    }
    __device__ __forceinline__ uint64_t u64(uint32_t o) const { return ((uint64_t)u32(o + 4) << 32) | u32(o); }
};

// the wave's batch [p, p + len) into its image, 16 bytes per lane per step
// from the aligned line p lies in; returns p's offset in the image
__device__ __forceinline__ uint32_t stage_batch(const uint8_t *p, uint32_t len, uint4 *img, uint32_t lane) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t sh = (uint32_t)(a & 15u);
    const uint4 *g = reinterpret_cast<const uint4 *>(a - sh);
    const uint32_t nq = (sh + len + 15u) >> 4;  // <= kStageQ - 1
    for (uint32_t q = lane; q < nq; q += 64) img[q] = g[q];
    return sh;
}

// the last of 64 ascending entries at or below r
__device__ __forceinline__ uint32_t last_le64(const uint32_t *pre, uint32_t r) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t w = 32; w > 0; w >>= 1)
        if (pre[k + w] <= r) k += w;
    return k;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t mx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t y = __shfl_xor(mx, o, 64);
        mx = y > mx ? y : mx;
    }
    return mx;
}

// batch b of the call: its bytes, or bad where off decreases, points past the
// buffer, or the length is outside [12, 4096]
__device__ __forceinline__ bool batch_span(const uint64_t *off, uint32_t b, uint64_t buf_len, uint64_t &o0,
                                           uint32_t &len) {
    o0 = off[b];
    const uint64_t o1 = off[b + 1];
    if (o1 < o0 || o1 > buf_len || o1 - o0 < DV_WIRE_HDR || o1 - o0 > kWireMsgMax) return false;
    len = (uint32_t)(o1 - o0);
    return true;
}

// ---- staging: a wave and the batch it holds
struct WaveBatch {
    uint32_t lane, wave, b, len;
    bool live, bad;  // a batch of the call; its span refused (nothing staged)
    Stage st;
};

// wave `wave` of the block takes batch b of the call's nb: nothing staged yet
__device__ __forceinline__ WaveBatch wave_batch(uint4 (*img)[kStageQ], uint32_t nb) {
    WaveBatch w;
    w.lane = threadIdx.x & 63, w.wave = threadIdx.x >> 6;
    w.b = blockIdx.x * kWireWave + w.wave;
    w.live = w.b < nb;
    w.bad = false;
    w.len = 0;
    w.st = Stage{reinterpret_cast<const uint32_t *>(img[w.wave]), 0};
    return w;
}

// The check's prologue: the wave's batch staged where its span is good.  Ends
// in a barrier: every wave of the block comes here, live or not.
__device__ __forceinline__ WaveBatch stage_wave_batch(uint4 (*img)[kStageQ], const uint8_t *buf, uint64_t buf_len,
                                                      const uint64_t *off, uint32_t first, uint32_t nb) {
    WaveBatch w = wave_batch(img, nb);
    uint64_t o0 = 0;
    w.bad = w.live && !batch_span(off, first + w.b, buf_len, o0, w.len);
    if (w.live && !w.bad) w.st.sh = stage_batch(buf + o0, w.len, img[w.wave], w.lane);
    __syncthreads();
    return w;
}

// The emit's prologue, for a block with a taken batch at least (the caller left
// with the whole block otherwise): batch b below `taken` was checked, its span
// and every field are good.  Ends in a barrier, as above.
__device__ __forceinline__ WaveBatch stage_taken_batch(uint4 (*img)[kStageQ], const uint8_t *buf,
                                                       const uint64_t *off, uint32_t first, uint32_t taken) {
    WaveBatch w = wave_batch(img, taken);
    if (w.live) {
        const uint64_t o0 = off[first + w.b];
        w.len = (uint32_t)(off[first + w.b + 1] - o0);
        w.st.sh = stage_batch(buf + o0, w.len, img[w.wave], w.lane);
    }
    __syncthreads();
    return w;
}

// ---- the chain
// message m as lane m keeps it: its offset and rtype; a CL_QRY's partition
// count, the offset `bo` behind its partitions and the count n its body named
struct Msg {
    uint32_t off, rt, np, n, bo;
};

// create_messages' asserts on {dest, src, count} (message.cpp:39-41)
template <class D>
__device__ __forceinline__ bool open_header(const Stage &st, const dv_wire_cfg &cfg, uint32_t &count) {
    count = st.u32(8);
    return st.u32(0) == cfg.node_id && st.u32(4) != cfg.node_id && count != 0 && count <= D::kStride;
}

// Every lane walks the batch's `count` messages; false for whatever
// dv_wire_open refuses in the chain, which must fill exactly `len` bytes.
// Every length is compared as the 64-bit count it is before it is multiplied:
// a count of 2^61 + 1 fails its limit, it never reaches n * 24.  body(bo, n)
// checks a CL_QRY's bytes from bo on, sets n and returns the message's end
// (0: refused).  Lane m is left message m in `mine`.
template <class D, class Body>
__device__ __forceinline__ bool walk_chain(const Stage &st, uint32_t len, uint32_t count, uint32_t lane, Msg &mine,
                                           Body body) {
    uint32_t pos = DV_WIRE_HDR;
    for (uint32_t m = 0; m < count; m++) {
        if (pos + (D::kRdone ? D::kHdr : D::kFixed) > len) return false;
        Msg g{pos, st.u32(pos), 0, 0, 0};
        // (a client's message is a query whatever it says: its rtype is tested beside its count, not in front)
        const bool query = !D::kRdone || g.rt == DV_WIRE_CL_QRY;
        if (D::kRdone && (st.u64(pos + kCalBatchId) == kNoBatchId || (!query && g.rt != DV_WIRE_RDONE) ||
                          (query && pos + D::kFixed > len)))
            return false;
        uint32_t end = pos + D::kHdr;
        if (query) {
            const uint64_t np = st.u64(pos + D::kHdr + 8);
            if (g.rt != DV_WIRE_CL_QRY || np > DV_TPCC_MAX_PARTS) return false;
            g.np = (uint32_t)np;
            g.bo = pos + D::kFixed + g.np * 8u;
            end = body(g.bo, g.n);
            if (!end) return false;
        }
        if (lane == m) mine = g;
        pos = end;
    }
    return pos == len;
}

// ---- a batch's flat loops: pre[m] things before message m, tot in all
// a partition named at or above part_cnt (mo: message m's offset)
template <class D>
__device__ __forceinline__ bool parts_wrong(const Stage &st, const uint32_t *pp, const uint16_t *mo, uint32_t tot_pp,
                                            uint32_t part_cnt, uint32_t lane) {
    bool wrong = false;
    for (uint32_t q = lane; q < tot_pp; q += 64) {
        const uint32_t m = last_le64(pp, q);
        wrong |= st.u64(mo[m] + D::kFixed + (q - pp[m]) * 8u) >= part_cnt;
    }
    return wrong;
}

// a request that is not RD / WR of a key inside the table (p2: the offset of message m's request count)
__device__ __forceinline__ bool requests_wrong(const Stage &st, const uint32_t *rq, const uint16_t *p2,
                                               uint32_t tot_rq, uint64_t table_size, uint32_t lane) {
    bool wrong = false;
    for (uint32_t r = lane; r < tot_rq; r += 64) {
        const uint32_t m = last_le64(rq, r);
        const uint32_t ro = p2[m] + 8u + (r - rq[m]) * kReqBytes;
        wrong |= st.u32(ro) > DV_WR || st.u64(ro + 8) >= table_size;
    }
    return wrong;
}

// the batch's requests in order -- consecutive lanes, consecutive accesses --
// from access a0 on; a request of message m belongs to txn t0 + txn_of(m)
template <class TxnOf>
__device__ __forceinline__ void emit_requests(const Stage &st, const uint32_t *rq, const uint16_t *p2, uint32_t tot_rq,
                                              uint32_t t0, uint32_t a0, const dv_wire_dev_out &out, uint32_t part_cnt,
                                              uint32_t lane, TxnOf txn_of) {
    for (uint32_t r = lane; r < tot_rq; r += 64) {
        const uint32_t m = last_le64(rq, r);
        const uint32_t ro = p2[m] + 8u + (r - rq[m]) * kReqBytes;
        const uint32_t acctype = st.u32(ro);
        const uint64_t key = st.u64(ro + 8);
        const uint32_t a = a0 + r;
        if (out.recs32) out.recs32[a] = (uint32_t)key | (acctype == DV_WR ? AR_WR : 0u);
        if (out.keys) {
            out.keys[a] = key;
            out.types[a] = (uint8_t)acctype;
            out.acc_txn[a] = t0 + txn_of(m);
        }
        if (out.owner) out.owner[a] = (uint8_t)(key % part_cnt);  // key_to_part
    }
}

// The YCSB check of a dialect up to its verdict, for every wave of the block
// (a barrier inside): the header, a cursor m0 below the count, the chain of
// queries of at most cfg.max_req (128) requests, then every partition and
// request.  True: the batch is refused whole.  (A bad batch's lanes hold zeros
// or a part of the chain: its tables are not read.)
struct YcsbTables {
    uint32_t rq[kWireWave][64], pp[kWireWave][64];  // requests / partitions before message m
    uint16_t mo[kWireWave][64], p2[kWireWave][64];  // message m's offset, its request count's
};
template <class D>
__device__ __forceinline__ bool ycsb_batch_bad(const WaveBatch &w, const dv_wire_cfg &cfg, uint32_t m0,
                                               YcsbTables &t, uint32_t &count, Msg &my, uint32_t &tot_rq) {
    const Stage &st = w.st;
    const bool parse = w.live && !w.bad;
    bool bad = w.bad;
    if (parse) {
        const uint32_t lim = cfg.max_req && cfg.max_req < kReqMax ? cfg.max_req : kReqMax;
        bad = !open_header<D>(st, cfg, count) || m0 >= count ||
              !walk_chain<D>(st, w.len, count, w.lane, my, [&](uint32_t bo, uint32_t &n) -> uint32_t {
                  if (bo + 8 > w.len) return 0;
                  const uint64_t n64 = st.u64(bo);
                  if (n64 > lim) return 0;
                  n = (uint32_t)n64;
                  const uint32_t end = bo + 8 + n * kReqBytes;
                  return end > w.len ? 0 : end;
              });
    }
    const uint32_t rq_in = wave_incl_sum(my.n, w.lane), pp_in = wave_incl_sum(my.np, w.lane);
    const uint32_t tot_pp = __shfl(pp_in, 63, 64);
    tot_rq = __shfl(rq_in, 63, 64);
    t.rq[w.wave][w.lane] = rq_in - my.n;
    t.pp[w.wave][w.lane] = pp_in - my.np;
    t.mo[w.wave][w.lane] = (uint16_t)my.off;
    t.p2[w.wave][w.lane] = (uint16_t)my.bo;
    __syncthreads();
    bool wrong = false;
    if (parse && !bad)
        wrong = parts_wrong<D>(st, t.pp[w.wave], t.mo[w.wave], tot_pp, cfg.part_cnt, w.lane) |
                requests_wrong(st, t.rq[w.wave], t.p2[w.wave], tot_rq, cfg.synth_table_size, w.lane);
    return bad || __any(wrong);
}

// ---- per batch and per txn
// what the check keeps of batch w.b: the offsets of a good batch's messages,
// its counts (a bad one counts nothing) and the first bad batch
template <class D>
__device__ __forceinline__ void keep_batch(const WireWs &ws, const WaveBatch &w, bool bad, uint32_t count,
                                           uint32_t my_off, uint32_t txns, uint32_t accs, uint32_t longest) {
    if (!bad && w.lane < count) ws.moff[(uint64_t)w.b * D::kStride + w.lane] = (uint16_t)my_off;
    if (w.lane == 0) {
        ws.bt[w.b] = bad ? 0u : txns;
        ws.ba[w.b] = bad ? 0u : accs;
        ws.bm[w.b] = bad ? (uint8_t)0 : (uint8_t)longest;
        if (bad) atomicMin(&ws.first[0], w.b);
    }
}

// the call's txns and accesses before batch b (after the scan)
__device__ __forceinline__ void batch_base(const WireWs &ws, uint32_t b, uint32_t &t0, uint32_t &a0) {
    t0 = ws.ct[b / kWireChunk] + ws.bt[b];
    a0 = ws.ca[b / kWireChunk] + ws.ba[b];
}

// a YCSB query at mo: client_startts, where its request count lies and the count
template <class D>
__device__ __forceinline__ void query_fields(const Stage &st, uint32_t mo, uint64_t &cst, uint32_t &p2, uint32_t &n) {
    cst = st.u64(mo + D::kHdr);
    p2 = mo + D::kFixed + st.u32(mo + D::kHdr + 8) * 8u;
    n = st.u32(p2);
}

// txn t: its boundary and what its reply needs
template <class Out>
__device__ __forceinline__ void emit_txn_fields(const Out &out, uint32_t t, uint32_t begin, uint64_t txn_id,
                                                uint64_t cst, uint32_t src) {
    out.txn_begin[t] = begin;
    if (out.txn_id) out.txn_id[t] = txn_id;
    if (out.client_startts) out.client_startts[t] = cst;
    if (out.return_node) out.return_node[t] = src;
}

// WorkerThread::get_next_txn_id for one worker (worker_thread.cpp:453-458)
__device__ __forceinline__ uint64_t worker_txn_id(const dv_wire_cfg &cfg, uint64_t k) {
    return cfg.node_id + (uint64_t)cfg.node_cnt * k;
}

// ---- the plan (one workgroup, every thread; both end in a barrier)
// The first batch of [0, nb) whose txns or accesses, added to those before it,
// pass the rooms, nb where none does: the running sums only grow, so it is
// the first batch of the first chunk that does not fit whole.  s_chunk = nc and
// s_cut = nb were set in front of a barrier; tot_t / tot_a: the chunks' totals.
__device__ __forceinline__ uint32_t first_overflow(const WireWs &ws, uint32_t nb, uint32_t nc, uint32_t tot_t,
                                                   uint32_t tot_a, uint64_t room_t, uint64_t room_a,
                                                   uint32_t *s_chunk, uint32_t *s_cut) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < nc; i += kBlock) {
        const uint32_t it = i + 1 < nc ? ws.ct[i + 1] : tot_t, ia = i + 1 < nc ? ws.ca[i + 1] : tot_a;
        if (it > room_t || ia > room_a) atomicMin(s_chunk, i);
    }
    __syncthreads();
    const uint32_t cc = *s_chunk;
    if (cc < nc) {
        const uint32_t base = cc * kWireChunk;
        const uint32_t n = nb - base < kWireChunk ? nb - base : kWireChunk;
        const uint32_t t0 = ws.ct[cc], a0 = ws.ca[cc];
        const uint32_t ch_t = (cc + 1 < nc ? ws.ct[cc + 1] : tot_t) - t0, ch_a = (cc + 1 < nc ? ws.ca[cc + 1] : tot_a) - a0;
        for (uint32_t j = tid; j < n; j += kBlock) {
            const uint32_t it = t0 + (j + 1 < n ? ws.bt[base + j + 1] : ch_t);
            const uint32_t ia = a0 + (j + 1 < n ? ws.ba[base + j + 1] : ch_a);
            if (it > room_t || ia > room_a) atomicMin(s_cut, base + j);
        }
    }
    __syncthreads();
    return *s_cut;
}

// the longest txn of batches [0, k) (s_max = 0 was set in front of a barrier)
__device__ __forceinline__ uint32_t longest_below(const WireWs &ws, uint32_t k, uint32_t *s_max) {
    const uint32_t full = k / kWireChunk;
    uint32_t mx = 0;
    for (uint32_t i = threadIdx.x; i < full; i += kBlock) mx = ws.cm[i] > mx ? ws.cm[i] : mx;
    for (uint32_t j = full * kWireChunk + threadIdx.x; j < k; j += kBlock) mx = ws.bm[j] > mx ? ws.bm[j] : mx;
    atomicMax(s_max, mx);
    __syncthreads();
    return *s_max;
}

// batches [0, k) of the call's nb hold this many of what (c, b) count per chunk and batch (tot: all nb)
__device__ __forceinline__ uint32_t sum_below(const uint32_t *c, const uint32_t *b, uint32_t k, uint32_t nb,
                                              uint32_t tot) {
    return k == nb ? tot : c[k / kWireChunk] + b[k];
}

}  // namespace

// Whatever dv_wire_open refuses makes the batch bad, whole.
__global__ __launch_bounds__(kBlock) void k_wire_check(dv_wire_cfg cfg, const uint8_t *__restrict__ buf,
                                                       uint64_t buf_len, const uint64_t *__restrict__ off,
                                                       uint32_t first, uint32_t nb, WireWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ YcsbTables s_t;
    const WaveBatch w = stage_wave_batch(s_img, buf, buf_len, off, first, nb);
    uint32_t count = 0, tot_rq;
    Msg my{};
    const bool bad = ycsb_batch_bad<Client>(w, cfg, 0, s_t, count, my, tot_rq);
    const uint32_t mx = wave_max(my.n);
    if (!w.live) return;
    keep_batch<Client>(ws, w, bad, count, my.off, count, tot_rq, mx);
}

// chunk blockIdx.x: the batches' counts become their prefixes inside the chunk
__global__ __launch_bounds__(kBlock) void k_wire_scan(WireWs ws, uint32_t nb) {
    __shared__ uint32_t lds4[4], s_max;
    const uint32_t base = blockIdx.x * kWireChunk;
    const uint32_t n = nb - base < kWireChunk ? nb - base : kWireChunk;
    if (threadIdx.x == 0) s_max = 0;
    uint32_t mx = 0;
    for (uint32_t j = threadIdx.x; j < n; j += kBlock) mx = ws.bm[base + j] > mx ? ws.bm[base + j] : mx;
    __syncthreads();
    atomicMax(&s_max, mx);
    const uint32_t t = block_chunk_scan256(ws.bt + base, n, lds4);
    const uint32_t a = block_chunk_scan256(ws.ba + base, n, lds4);
    __syncthreads();
    if (threadIdx.x == 0) {
        ws.ct[blockIdx.x] = t;
        ws.ca[blockIdx.x] = a;
        ws.cm[blockIdx.x] = s_max;
    }
}

// One workgroup.  Batches are taken up to the first stopper in batch order: a
// malformed batch (k_wire_check's ws.first[0]), or the first that does not fit
// the capacities (first_overflow; a bad batch counts nothing: it never is the
// capacity cut).  Of the call's out it takes what it reads: the capacities,
// the boundaries, the count word -- the same for every dialect's out.
__global__ __launch_bounds__(kBlock) void k_wire_plan(WireWs ws, uint32_t first, uint32_t nb, uint32_t n_batches,
                                                      uint32_t nc, uint32_t max_txn, uint64_t max_acc,
                                                      uint32_t *__restrict__ txn_begin,
                                                      uint32_t *__restrict__ n_acc_dev, uint64_t next_txn) {
    __shared__ uint32_t lds4[4], s_chunk, s_cut, s_max;
    if (threadIdx.x == 0) {
        s_chunk = nc;
        s_cut = nb;
        s_max = 0;
    }
    const uint32_t tot_t = block_chunk_scan256(ws.ct, nc, lds4);
    const uint32_t tot_a = block_chunk_scan256(ws.ca, nc, lds4);
    __syncthreads();
    const uint32_t cut = first_overflow(ws, nb, nc, tot_t, tot_a, max_txn, max_acc, &s_chunk, &s_cut);
    const uint32_t fb = ws.first[0];
    const uint32_t k = fb < cut ? fb : cut;  // batches taken (<= nb)
    const uint32_t longest = longest_below(ws, k, &s_max);
    if (threadIdx.x != 0) return;
    const uint32_t n_txn = sum_below(ws.ct, ws.bt, k, nb, tot_t), n_acc = sum_below(ws.ca, ws.ba, k, nb, tot_a);
    int32_t status = DV_OK;
    if (fb < nb && fb <= cut) status = DV_ERR_ARG;                // the malformed batch comes first
    else if (cut < nb) status = cut ? DV_WIRE_MORE : DV_ERR_ARG;  // (the first batch: it would never fit)
    else if (first + nb < n_batches) status = DV_WIRE_MORE;       // (the call's window of max_txn + 1 batches)
    dv_wire_dev_result r;
    r.status = status;
    r.n_taken = first + k;
    r.n_txn = n_txn;
    r.max_txn_acc = longest;
    r.n_acc = n_acc;
    r.next_txn = next_txn + n_txn;
    *ws.res = r;
    txn_begin[n_txn] = n_acc;  // (n_txn <= max_txn)
    *n_acc_dev = n_acc;
}

// the taken batches (below the plan's n_taken), a wave each: lane m message
// m's boundary and reply fields, then all lanes the batch's requests
__global__ __launch_bounds__(kBlock) void k_wire_emit(dv_wire_cfg cfg, const uint8_t *__restrict__ buf,
                                                      const uint64_t *__restrict__ off, uint32_t first,
                                                      dv_wire_dev_out out, uint64_t next_txn, WireWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint32_t s_rq[kWireWave][64];
    __shared__ uint16_t s_p2[kWireWave][64];
    const uint32_t taken = ws.res->n_taken - first;
    if (blockIdx.x * kWireWave >= taken) return;
    const WaveBatch w = stage_taken_batch(s_img, buf, off, first, taken);
    const uint32_t lane = w.lane, wave = w.wave;
    uint32_t count = 0, src = 0, my_n = 0, my_p2 = 0, t0 = 0, a0 = 0;
    uint64_t cst = 0;
    if (w.live) {
        src = w.st.u32(4);
        count = w.st.u32(8);
        batch_base(ws, w.b, t0, a0);
        if (lane < count) query_fields<Client>(w.st, ws.moff[(uint64_t)w.b * Client::kStride + lane], cst, my_p2, my_n);
    }
    const uint32_t rq_in = wave_incl_sum(my_n, lane);
    const uint32_t tot_rq = __shfl(rq_in, 63, 64);
    s_rq[wave][lane] = rq_in - my_n;
    s_p2[wave][lane] = (uint16_t)my_p2;
    __syncthreads();
    if (!w.live) return;
    if (lane < count)
        emit_txn_fields(out, t0 + lane, a0 + rq_in - my_n, worker_txn_id(cfg, next_txn + t0 + lane), cst, src);
    emit_requests(w.st, s_rq[wave], s_p2[wave], tot_rq, t0, a0, out, cfg.part_cnt, lane,
                  [](uint32_t m) { return m; });
}

// the check, the scan and the plan of a client dialect's batches, `check` launched with the kernel's own arguments
template <class Check>
static void launch_client_plan(hipStream_t s, uint32_t first, uint32_t nb, uint32_t n_batches, uint32_t max_txn,
                               uint64_t max_acc, uint32_t *txn_begin, uint32_t *n_acc_dev, uint64_t next_txn,
                               const WireWs &ws, Check check) {
    const uint32_t nc = (nb + kWireChunk - 1) / kWireChunk;
    (void)hipMemsetAsync(ws.first, 0xFF, 2 * sizeof(uint32_t), s);  // kNoBatch
    static_assert(kNoBatch == 0xFFFFFFFFu, "the memset's value");
    if (nb) {
        check((nb + kWireWave - 1) / kWireWave);
        DV_LAUNCH(k_wire_scan, nc, kBlock, 0, s, ws, nb);
    }
    DV_LAUNCH(k_wire_plan, 1, kBlock, 0, s, ws, first, nb, n_batches, nc, max_txn, max_acc, txn_begin, n_acc_dev,
              next_txn);
}

void launch_wire_plan(hipStream_t s, const dv_wire_cfg &cfg, const uint8_t *buf, uint64_t buf_len,
                      const uint64_t *off, uint32_t first, uint32_t nb, uint32_t n_batches,
                      const dv_wire_dev_out &out, uint64_t next_txn, const WireWs &ws) {
    launch_client_plan(s, first, nb, n_batches, out.max_txn, out.max_acc, out.txn_begin, out.n_acc_dev, next_txn, ws,
                       [&](uint32_t grid) {
                           DV_LAUNCH(k_wire_check, grid, kBlock, 0, s, cfg, buf, buf_len, off, first, nb, ws);
                       });
}

void launch_wire_emit(hipStream_t s, const dv_wire_cfg &cfg, const uint8_t *buf, const uint64_t *off,
                      uint32_t first, uint32_t nb, const dv_wire_dev_out &out, uint64_t next_txn,
                      const WireWs &ws) {
    if (!nb) return;
    DV_LAUNCH(k_wire_emit, (nb + kWireWave - 1) / kWireWave, kBlock, 0, s, cfg, buf, off, first, out, next_txn, ws);
}

// ---- TPC-C client batches (dv_wire_ingest_device_tpcc): the same four
// launches, k_wire_scan and k_wire_plan as they are.  A TPCCClientQueryMessage
// is 199 + 8 np + 24 n bytes (Client::kFixed, the partitions, kTpccBody up to
// the item count, the items, kTpccTail) and expands -- dv_tpcc_expand's lists,
// a closed form of the message's fields per access -- to 3 accesses (Payment)
// or 3 + 2 ol_cnt (NewOrder).  The knobs the lists follow come by value.
namespace {

constexpr uint32_t kTpccBody = 89;   // txn_type, w_id, d_id, c_id, d_w_id, c_w_id, c_d_id, c_last[16], h_amount,
                                     // by_last_name, the item count
constexpr uint32_t kTpccTail = 18;   // rbk, remote, ol_cnt, o_entry_d
constexpr uint32_t kItemBytes = 24;  // sizeof(Item_no)
constexpr uint32_t kTpccLast = 56, kTpccAmount = 72, kTpccByName = 80, kTpccN = 81;  // body offsets
constexpr uint64_t kOperandMax = (1ull << 56) - 1;

// 1 <= v <= bound, v the 64-bit field it is
__device__ __forceinline__ bool in_1_to(uint64_t v, uint32_t bound) { return v - 1 < (uint64_t)bound; }
// a zero byte somewhere in v
__device__ __forceinline__ bool has_nul(uint64_t v) {
    return ((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) != 0;
}
// custNPKey (tpcc_helper.cpp:35-43) of the name in c_last[16] (lo, hi: its
// bytes, a NUL among them): the host's `char` arithmetic, a byte below 'A' or
// at 0x80 and above sign-extended; the district's 10 bits overflow past
// warehouse 102 (H8), kept
__device__ __forceinline__ uint64_t cust_np_key(uint64_t lo, uint64_t hi, uint64_t dist) {
    uint64_t key = 0;
    bool open = true;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t ch = (uint32_t)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xFFu);
        open = open && ch != 0;
        if (open) key = (key << 1) + (uint64_t)(int64_t)((int32_t)(int8_t)ch - (int32_t)'A');
    }
    return (key << 10) + dist;
}

// walk_chain's body of a TPC-C query at bo: its item count (at most 62, the
// 64-bit count it is) and its end behind the items and the tail; 0: refused
__device__ __forceinline__ uint32_t tpcc_body_end(const Stage &st, uint32_t len, uint32_t bo, uint32_t &n) {
    if (bo + kTpccBody > len) return 0;
    const uint64_t n64 = st.u64(bo + kTpccN);
    if (n64 > DV_TPCC_MAX_OL) return 0;
    n = (uint32_t)n64;
    const uint32_t end = bo + kTpccBody + n * kItemBytes + kTpccTail;
    return end > len ? 0 : end;
}

// dv_tpcc_expand's checks of a query's fixed fields (body at bo, n items):
// true where it refuses them.  acc: the accesses it expands to, it: the items
// still to check -- a NewOrder's (a Payment's are skipped unchecked).
__device__ __forceinline__ bool tpcc_fields_wrong(const Stage &st, const dv_tpcc_params &tp, uint32_t bo, uint32_t n,
                                                  uint32_t &acc, uint32_t &it) {
    const uint64_t tt = st.u64(bo), wh = st.u64(bo + 8), d = st.u64(bo + 16), c = st.u64(bo + 24);
    bool wrong = !in_1_to(wh, tp.num_wh) || !in_1_to(d, tp.dist_per_wh);
    if (tt == 1) {
        wrong |= !in_1_to(st.u64(bo + 40), tp.num_wh) || !in_1_to(st.u64(bo + 48), tp.dist_per_wh) ||
                 st.u64(bo + kTpccAmount) > kOperandMax;
        if ((st.u32(bo + kTpccByName) & 0xFFu) != 0)
            wrong |= !has_nul(st.u64(bo + kTpccLast)) && !has_nul(st.u64(bo + kTpccLast + 8));
        else
            wrong |= !in_1_to(c, tp.cust_per_dist);
        acc = 3;
    } else if (tt == 2) {
        // the txn manager walks items[0 .. ol_cnt): the list must hold them, one at least
        const uint64_t ol_cnt = st.u64(bo + kTpccBody + n * kItemBytes + 2);
        wrong |= ol_cnt != n || n == 0 || !in_1_to(c, tp.cust_per_dist);
        acc = 3 + 2 * n;
        it = n;
    } else {
        wrong = true;
    }
    return wrong;
}

// the batch's NewOrder items, one flat range (it[m]: items before message m,
// io[m]: its first item's offset): an item outside the tables, an operand
// above 56 bits
__device__ __forceinline__ bool tpcc_items_wrong(const Stage &st, const dv_tpcc_params &tp, const uint32_t *it,
                                                 const uint16_t *io, uint32_t tot_it, uint32_t lane) {
    bool wrong = false;
    for (uint32_t q = lane; q < tot_it; q += 64) {
        const uint32_t m = last_le64(it, q);
        const uint32_t o = io[m] + (q - it[m]) * kItemBytes;
        wrong |= !in_1_to(st.u64(o), tp.max_items) || !in_1_to(st.u64(o + 8), tp.num_wh) ||
                 st.u64(o + 16) > kOperandMax;
    }
    return wrong;
}

// what a checked query's lane keeps for the expansion: the keys of its three
// leading accesses, h_amount, mt = Payment | by name << 1 | w_id's partition
// << 8 | c_w_id's << 16, its txn type, access count and first item's offset
struct TpccLead {
    uint64_t k0, k1, k2, h;
    uint32_t tt, mt, acc, io;
};
__device__ __forceinline__ TpccLead tpcc_lead(const Stage &st, const dv_tpcc_params &tp, uint32_t bo) {
    TpccLead l{};
    l.io = bo + kTpccBody;
    l.tt = st.u32(bo);
    // (validated: every id below its 32-bit bound)
    const uint32_t w = st.u32(bo + 8), d = st.u32(bo + 16), c = st.u32(bo + 24);
    const uint64_t dist = (uint64_t)w * tp.dist_per_wh + d;
    const uint32_t pw = (w - 1) % tp.part_cnt;  // wh_to_part
    l.k0 = w;
    if (l.tt == 1) {
        const uint32_t c_w = st.u32(bo + 40), c_d = st.u32(bo + 48);
        const uint64_t c_dist = (uint64_t)c_w * tp.dist_per_wh + c_d;
        const bool by_name = (st.u32(bo + kTpccByName) & 0xFFu) != 0;
        l.h = st.u64(bo + kTpccAmount);
        l.k1 = dist;
        l.k2 = by_name ? cust_np_key(st.u64(bo + kTpccLast), st.u64(bo + kTpccLast + 8), c_dist)
                       : c_dist * tp.cust_per_dist + c;
        l.mt = 1u | (by_name ? 2u : 0u) | ((pw & 0xFFu) << 8) | ((((c_w - 1) % tp.part_cnt) & 0xFFu) << 16);
        l.acc = 3;
    } else {
        l.k1 = dist * tp.cust_per_dist + c;
        l.k2 = dist;
        l.mt = (pw & 0xFFu) << 8;
        l.acc = 3 + 2 * st.u32(bo + kTpccN);
    }
    return l;
}

// a wave's table of its messages' leads (LDS), ac[m]: accesses before message m
struct TpccLds {
    uint64_t (*hk)[3], *h;
    uint32_t *ac, *mt;
    uint16_t *io;
    __device__ __forceinline__ void keep(uint32_t lane, const TpccLead &l, uint32_t ac_before) const {
        ac[lane] = ac_before;
        io[lane] = (uint16_t)l.io;
        mt[lane] = l.mt;
        h[lane] = l.h;
        hk[lane][0] = l.k0;
        hk[lane][1] = l.k1;
        hk[lane][2] = l.k2;
    }
};

// the batch's tot_ac accesses in order from access a0 on -- consecutive lanes,
// consecutive accesses, access j of message m from m's lead and items alone
// (dv_tpcc_expand's lists); an access of message m belongs to txn t0 + txn_of(m)
template <class TxnOf>
__device__ __forceinline__ void emit_tpcc_accesses(const Stage &st, const dv_tpcc_params &tp, const TpccLds &t,
                                                   uint32_t tot_ac, uint32_t t0, uint32_t a0,
                                                   const dv_wire_tpcc_dev_out &out, uint32_t lane, TxnOf txn_of) {
    for (uint32_t r = lane; r < tot_ac; r += 64) {
        const uint32_t m = last_le64(t.ac, r);
        const uint32_t j = r - t.ac[m], mt = t.mt[m];
        uint64_t key, arg;
        uint32_t type, table, own = (mt >> 8) & 0xFFu;
        if (j < 3) {
            key = t.hk[m][j];
            if (mt & 1u) {  // run_payment_0..5: WAREHOUSE, DISTRICT, CUSTOMER (by id or through the name index)
                const uint32_t op = j == 0 ? (tp.wh_update ? DV_TOP_PAY_WH : DV_TOP_NONE)
                                           : (j == 1 ? DV_TOP_PAY_DIST : DV_TOP_PAY_CUST);
                type = j == 0 && !tp.wh_update ? DV_RD : DV_WR;
                table = j == 0 ? DV_TPCC_WAREHOUSE
                               : (j == 1 ? DV_TPCC_DISTRICT : ((mt & 2u) ? DV_TPCC_CUST_LAST : DV_TPCC_CUSTOMER));
                arg = (uint64_t)op << 56 | t.h[m];
                if (j == 2) own = (mt >> 16) & 0xFFu;
            } else {  // new_order_0..5: WAREHOUSE RD, CUSTOMER RD, DISTRICT WR
                type = j == 2 ? DV_WR : DV_RD;
                table = j == 0 ? DV_TPCC_WAREHOUSE : (j == 1 ? DV_TPCC_CUSTOMER : DV_TPCC_DISTRICT);
                arg = j == 2 ? (uint64_t)DV_TOP_NO_DIST << 56 : 0;
            }
        } else {  // new_order_6..9: ITEM RD, STOCK WR of item (j - 3) / 2, both with the supply warehouse
            const uint32_t io = t.io[m] + ((j - 3) >> 1) * kItemBytes;
            const uint32_t i_id = st.u32(io), sw = st.u32(io + 8);
            own = ((sw - 1) % tp.part_cnt) & 0xFFu;
            if (j & 1u) {
                key = i_id;
                type = DV_RD;
                table = DV_TPCC_ITEM;
                arg = 0;
            } else {
                key = (uint64_t)sw * tp.max_items + i_id;
                type = DV_WR;
                table = DV_TPCC_STOCK;
                arg = (uint64_t)DV_TOP_NO_STOCK << 56 | st.u64(io + 16);
            }
        }
        const uint32_t a = a0 + r;
        out.keys[a] = key;
        out.types[a] = (uint8_t)type;
        out.acc_txn[a] = t0 + txn_of(m);
        out.tables[a] = (uint8_t)table;
        out.args[a] = arg;
        if (out.owner) out.owner[a] = (uint8_t)own;
    }
}

}  // namespace

// dv_wire_open for a TPC-C cfg: read_client_part, read_tpcc, then
// dv_tpcc_expand's checks.  Lane m checks message m's fixed fields; the
// batch's NewOrder items are one flat range all lanes check.  Every count and
// id is compared as the 64-bit value it is before it is multiplied or narrowed.
__global__ __launch_bounds__(kBlock) void k_wire_check_tpcc(dv_wire_cfg cfg, dv_tpcc_params tp,
                                                            const uint8_t *__restrict__ buf, uint64_t buf_len,
                                                            const uint64_t *__restrict__ off, uint32_t first,
                                                            uint32_t nb, WireWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint32_t s_it[kWireWave][64], s_pp[kWireWave][64];  // items to check / partitions before message m
    __shared__ uint16_t s_mo[kWireWave][64], s_io[kWireWave][64];  // message m's offset, its first item's
    const WaveBatch w = stage_wave_batch(s_img, buf, buf_len, off, first, nb);
    const Stage &st = w.st;
    const uint32_t lane = w.lane, wave = w.wave;
    const bool parse = w.live && !w.bad;
    bool bad = w.bad;
    uint32_t count = 0;
    Msg my{};
    if (parse)
        bad = !open_header<Client>(st, cfg, count) ||
              !walk_chain<Client>(st, w.len, count, lane, my, [&](uint32_t bo, uint32_t &n) -> uint32_t {
                  return tpcc_body_end(st, w.len, bo, n);
              });
    // message m's fixed fields (a Payment's items are skipped unchecked)
    bool wrong = false;
    uint32_t my_acc = 0, my_it = 0;
    if (parse && !bad && lane < count) wrong = tpcc_fields_wrong(st, tp, my.bo, my.n, my_acc, my_it);
    // (a bad batch's lanes hold zeros or a part of the chain: its tables are not read)
    const uint32_t it_in = wave_incl_sum(my_it, lane), pp_in = wave_incl_sum(my.np, lane);
    const uint32_t ac_in = wave_incl_sum(my_acc, lane);
    const uint32_t tot_it = __shfl(it_in, 63, 64), tot_pp = __shfl(pp_in, 63, 64), tot_ac = __shfl(ac_in, 63, 64);
    const uint32_t mx = wave_max(my_acc);  // (at most 3 + 2 * 62)
    s_it[wave][lane] = it_in - my_it;
    s_pp[wave][lane] = pp_in - my.np;
    s_mo[wave][lane] = (uint16_t)my.off;
    s_io[wave][lane] = (uint16_t)(my.bo + kTpccBody);
    __syncthreads();
    if (parse && !bad) {
        wrong |= parts_wrong<Client>(st, s_pp[wave], s_mo[wave], tot_pp, cfg.part_cnt, lane);
        wrong |= tpcc_items_wrong(st, tp, s_it[wave], s_io[wave], tot_it, lane);
    }
    bad = bad || __any(wrong);
    if (!w.live) return;
    keep_batch<Client>(ws, w, bad, count, my.off, count, tot_ac, mx);
}

// the taken batches, a wave each: lane m message m's boundary, txn type, reply
// fields and the keys of its three leading accesses; then all lanes the
// batch's accesses in order -- consecutive lanes, consecutive accesses, access
// r of message m from m's fields alone (dv_tpcc_expand's lists)
__global__ __launch_bounds__(kBlock) void k_wire_emit_tpcc(dv_wire_cfg cfg, dv_tpcc_params tp,
                                                           const uint8_t *__restrict__ buf,
                                                           const uint64_t *__restrict__ off, uint32_t first,
                                                           dv_wire_tpcc_dev_out out, uint64_t next_txn, WireWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint64_t s_hk[kWireWave][64][3], s_h[kWireWave][64];  // message m's leading keys, its h_amount
    __shared__ uint32_t s_ac[kWireWave][64];                         // accesses before message m
    __shared__ uint16_t s_io[kWireWave][64];                         // message m's first item
    __shared__ uint32_t s_mt[kWireWave][64];  // Payment | by name << 1 | w_id's partition << 8 | c_w_id's << 16
    const uint32_t taken = ws.res->n_taken - first;
    if (blockIdx.x * kWireWave >= taken) return;
    const WaveBatch wb = stage_taken_batch(s_img, buf, off, first, taken);
    const Stage &st = wb.st;
    const uint32_t lane = wb.lane, wave = wb.wave;
    uint32_t count = 0, src = 0, t0 = 0, a0 = 0;
    uint64_t cst = 0;
    TpccLead my{};
    if (wb.live) {
        src = st.u32(4);
        count = st.u32(8);
        batch_base(ws, wb.b, t0, a0);
        if (lane < count) {
            const uint32_t mo = ws.moff[(uint64_t)wb.b * Client::kStride + lane];
            cst = st.u64(mo + Client::kHdr);
            my = tpcc_lead(st, tp, mo + Client::kFixed + st.u32(mo + Client::kHdr + 8) * 8u);
        }
    }
    const uint32_t ac_in = wave_incl_sum(my.acc, lane);
    const uint32_t tot_ac = __shfl(ac_in, 63, 64);
    const TpccLds t{s_hk[wave], s_h[wave], s_ac[wave], s_mt[wave], s_io[wave]};
    t.keep(lane, my, ac_in - my.acc);
    __syncthreads();
    if (!wb.live) return;
    if (lane < count) {
        const uint32_t txn = t0 + lane;
        if (out.txn_type) out.txn_type[txn] = (uint8_t)my.tt;
        emit_txn_fields(out, txn, a0 + ac_in - my.acc, worker_txn_id(cfg, next_txn + txn), cst, src);
    }
    emit_tpcc_accesses(st, tp, t, tot_ac, t0, a0, out, lane, [](uint32_t m) { return m; });
}

// cfg as the TPC-C kernels get it: tpcc is a host pointer, the knobs go by value
static dv_wire_cfg without_tpcc(dv_wire_cfg cfg) {
    cfg.tpcc = nullptr;
    return cfg;
}

void launch_wire_plan_tpcc(hipStream_t s, const dv_wire_cfg &cfg, const dv_tpcc_params &tp, const uint8_t *buf,
                           uint64_t buf_len, const uint64_t *off, uint32_t first, uint32_t nb, uint32_t n_batches,
                           const dv_wire_tpcc_dev_out &out, uint64_t next_txn, const WireWs &ws) {
    launch_client_plan(s, first, nb, n_batches, out.max_txn, out.max_acc, out.txn_begin, out.n_acc_dev, next_txn, ws,
                       [&](uint32_t grid) {
                           DV_LAUNCH(k_wire_check_tpcc, grid, kBlock, 0, s, without_tpcc(cfg), tp, buf, buf_len, off,
                                     first, nb, ws);
                       });
}

void launch_wire_emit_tpcc(hipStream_t s, const dv_wire_cfg &cfg, const dv_tpcc_params &tp, const uint8_t *buf,
                           const uint64_t *off, uint32_t first, uint32_t nb, const dv_wire_tpcc_dev_out &out,
                           uint64_t next_txn, const WireWs &ws) {
    if (!nb) return;
    DV_LAUNCH(k_wire_emit_tpcc, (nb + kWireWave - 1) / kWireWave, kBlock, 0, s, without_tpcc(cfg), tp, buf, off, first,
              out, next_txn, ws);
}

// ---- CALVIN sequencer streams (dv_wire_ingest_device_calvin): the same four
// launches, kernels of the same shape over the Calvin dialect.  The header
// carries batch_id (84 bytes), an RDONE is the header alone, and the stream is
// cut at a message: an mbuf's run is its messages from the cursor that name
// the epoch's batch E, and an epoch ends inside the first mbuf whose run does
// not reach its end.  The check cannot know E (it may be the first mbuf's
// own), so it measures every mbuf's run against the id of its own first
// message; the scan, which knows E, drops the mbufs that lead with another id
// and finds the first cut.
namespace {

constexpr uint32_t kRunLater = 1, kRunEarlier = 2;  // WireCalvinWs::bflag

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, uint32_t src) {
    return ((uint64_t)__shfl((uint32_t)(v >> 32), (int)src, 64) << 32) | __shfl((uint32_t)v, (int)src, 64);
}

// The run of a checked mbuf and what the check keeps of it, for every lane of
// the wave (lane m: message m in `my`, acc the accesses it becomes as a txn):
// the lanes from the cursor m0 up to the first whose batch id differs from the
// cursor's.  The counts are the run's alone, whatever the mbuf holds behind it.
__device__ __forceinline__ void keep_run(const WireCalvinWs &ws, const WaveBatch &w, bool bad, uint32_t count,
                                         uint32_t m0, const Msg &my, uint32_t acc) {
    const uint32_t lane = w.lane, b = w.b;
    const uint64_t my_bid = !bad && lane < count ? w.st.u64(my.off + kCalBatchId) : 0;
    // the run: lanes [m0, rend), the first lane behind the cursor whose id is not the cursor's
    const uint64_t lead = shfl_u64(my_bid, m0 & 63u);
    const uint64_t differ = __ballot(lane >= m0 && lane < count && my_bid != lead);
    const uint32_t rend = differ ? (uint32_t)__ffsll((long long)differ) - 1u : count;
    const bool in_run = lane >= m0 && lane < rend;
    const bool is_q = in_run && my.rt == DV_WIRE_CL_QRY;
    const uint32_t txns = (uint32_t)__popcll(__ballot(is_q));
    const uint32_t rdones = (uint32_t)__popcll(__ballot(in_run && my.rt == DV_WIRE_RDONE));
    const uint32_t run_n = is_q ? acc : 0u;
    const uint32_t accs = __shfl(wave_incl_sum(run_n, lane), 63, 64);
    const uint32_t mx = wave_max(run_n);
    const uint64_t behind = shfl_u64(my_bid, rend & 63u);
    if (!w.live) return;
    keep_batch<Calvin>(ws, w, bad, count, my.off, txns, accs, mx);
    if (lane == 0) {
        ws.br[b] = bad ? 0u : rdones;
        ws.bid[b] = bad ? kNoBatchId : lead;
        ws.brun[b] = bad ? (uint8_t)0 : (uint8_t)(rend - m0);
        ws.bflag[b] = bad || rend >= count ? (uint8_t)0 : (uint8_t)(behind > lead ? kRunLater : kRunEarlier);
    }
}

}  // namespace

// Whatever dv_wire_open refuses under a CALVIN cfg makes the mbuf bad, whole,
// and so does a cursor at or past its count.  Lane m keeps message m's rtype
// and batch id: the run is the lanes from the cursor up to the first whose id
// differs from the cursor's.
__global__ __launch_bounds__(kBlock) void k_wire_check_calvin(dv_wire_cfg cfg, const uint8_t *__restrict__ buf,
                                                              uint64_t buf_len, const uint64_t *__restrict__ off,
                                                              uint32_t first, uint32_t msg0, uint32_t nb,
                                                              WireCalvinWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ YcsbTables s_t;
    const WaveBatch w = stage_wave_batch(s_img, buf, buf_len, off, first, nb);
    const uint32_t m0 = w.b == 0 ? msg0 : 0;  // the cursor's message (the window's first mbuf is the cursor's)
    uint32_t count = 0, tot_rq;
    Msg my{};
    // every message of the mbuf, in the run or not: it is refused whole
    const bool bad = ycsb_batch_bad<Calvin>(w, cfg, m0, s_t, count, my, tot_rq);
    keep_run(ws, w, bad, count, m0, my, my.n);  // (a query's requests are its accesses)
}

// chunk blockIdx.x: an mbuf that leads with another id than E has an empty run
// (its counts go); the first such mbuf, or the first whose run ends inside it,
// is where the batch ends; then the counts become prefixes inside the chunk.
// E by value, or -- none yet -- the id the check read at the cursor.
__global__ __launch_bounds__(kBlock) void k_wire_scan_calvin(WireCalvinWs ws, uint32_t nb, uint64_t batch_id) {
    __shared__ uint32_t lds4[4], s_max;
    const uint64_t E = batch_id != kNoBatchId ? batch_id : ws.bid[0];
    const uint32_t base = blockIdx.x * kWireChunk;
    const uint32_t n = nb - base < kWireChunk ? nb - base : kWireChunk;
    if (threadIdx.x == 0) s_max = 0;
    uint32_t mx = 0, cut = kNoBatch;
    for (uint32_t j = threadIdx.x; j < n; j += kBlock) {
        const uint32_t g = base + j;
        if (ws.bid[g] != E) {
            ws.bt[g] = ws.ba[g] = ws.br[g] = 0;
            ws.bm[g] = 0;
            cut = g < cut ? g : cut;
        } else {
            if (ws.bflag[g]) cut = g < cut ? g : cut;
            mx = ws.bm[g] > mx ? ws.bm[g] : mx;
        }
    }
    if (cut != kNoBatch) atomicMin(&ws.first[1], cut);
    __syncthreads();  // (the counts dropped above are read by other threads below)
    atomicMax(&s_max, mx);
    const uint32_t t = block_chunk_scan256(ws.bt + base, n, lds4);
    const uint32_t a = block_chunk_scan256(ws.ba + base, n, lds4);
    const uint32_t r = block_chunk_scan256(ws.br + base, n, lds4);
    __syncthreads();
    if (threadIdx.x == 0) {
        ws.ct[blockIdx.x] = t;
        ws.ca[blockIdx.x] = a;
        ws.cr[blockIdx.x] = r;
        ws.cm[blockIdx.x] = s_max;
    }
}

// One workgroup.  Mbuf by mbuf the first stopper decides, and inside an mbuf a
// malformed one comes before its capacity test, which comes before the end of
// its run: the minimum of the first bad mbuf, the first whose run, added to
// the epoch's and the runs' before it, passes the capacities (the running sums
// only grow; past the batch's end they count mbufs never reached, and the
// minimum ignores them) and the first where the batch ends.  Of the call's out
// it takes what it reads, as k_wire_plan does: the same for both workloads' out.
__global__ __launch_bounds__(kBlock) void k_wire_plan_calvin(WireCalvinWs ws, uint32_t nb, uint32_t n_batches,
                                                             uint32_t nc, uint32_t max_txn, uint64_t max_acc,
                                                             uint32_t *__restrict__ txn_begin,
                                                             uint32_t *__restrict__ n_acc_dev,
                                                             dv_wire_calvin_pos pos) {
    __shared__ uint32_t lds4[4], s_chunk, s_cut, s_max;
    if (threadIdx.x == 0) {
        s_chunk = nc;
        s_cut = nb;
        s_max = 0;
    }
    const uint32_t tot_t = block_chunk_scan256(ws.ct, nc, lds4);
    const uint32_t tot_a = block_chunk_scan256(ws.ca, nc, lds4);
    const uint32_t tot_r = block_chunk_scan256(ws.cr, nc, lds4);
    __syncthreads();
    // (checked: the rooms are not negative)
    const uint32_t cut = first_overflow(ws, nb, nc, tot_t, tot_a, max_txn - pos.n_txn, max_acc - pos.n_acc,
                                        &s_chunk, &s_cut);
    const uint32_t fb = nb ? ws.first[0] : kNoBatch, fe = nb ? ws.first[1] : kNoBatch;
    uint32_t s = fb < cut ? fb : cut;
    s = fe < s ? fe : s;  // (<= nb)
    uint32_t stop;
    if (s == nb) stop = pos.batch + nb < n_batches ? DV_WIRE_STOP_WINDOW : DV_WIRE_STOP_END;
    else if (s == fb) stop = DV_WIRE_STOP_MALFORMED;
    else if (s == cut) stop = DV_WIRE_STOP_CAPACITY;
    else stop = DV_WIRE_STOP_BATCH;  // (or STALE, below)
    const uint64_t E = pos.batch_id != kNoBatchId ? pos.batch_id : (nb ? ws.bid[0] : kNoBatchId);
    const uint32_t m0 = s == 0 ? pos.msg : 0;
    uint32_t run = 0;
    if (stop == DV_WIRE_STOP_BATCH) {
        const uint64_t id = ws.bid[s];
        if (id == E) {
            run = ws.brun[s];
            if (ws.bflag[s] == kRunEarlier) stop = DV_WIRE_STOP_STALE;
        } else if (id < E) {
            stop = DV_WIRE_STOP_STALE;
        }
    }
    const bool ends = stop == DV_WIRE_STOP_BATCH || stop == DV_WIRE_STOP_STALE;
    const uint32_t k = s + (ends ? 1u : 0u);  // mbufs whose runs are taken (<= nb)
    const uint32_t longest = longest_below(ws, k, &s_max);
    if (threadIdx.x != 0) return;
    const uint32_t n_txn = pos.n_txn + sum_below(ws.ct, ws.bt, k, nb, tot_t);
    const uint64_t n_acc = pos.n_acc + sum_below(ws.ca, ws.ba, k, nb, tot_a);
    WireCalvinRes r;
    r.pos.batch = stop == DV_WIRE_STOP_END ? n_batches : pos.batch + s;
    r.pos.msg = s == nb ? 0u : m0 + run;
    r.pos.n_txn = n_txn;
    r.pos.rdone = pos.rdone + sum_below(ws.cr, ws.br, k, nb, tot_r);
    r.pos.n_acc = n_acc;
    r.pos.batch_id = s > 0 || run > 0 ? E : pos.batch_id;  // (every mbuf taken whole holds a message behind the cursor)
    r.pos.max_txn_acc = longest > pos.max_txn_acc ? longest : pos.max_txn_acc;
    r.pos.stop = stop;
    r.status = stop == DV_WIRE_STOP_END ? DV_OK
               : stop == DV_WIRE_STOP_MALFORMED || stop == DV_WIRE_STOP_STALE ? DV_ERR_ARG
               : stop == DV_WIRE_STOP_CAPACITY && n_txn == 0 ? DV_ERR_ARG
                                                             : DV_WIRE_MORE;
    r.n_emit = ends && run == 0 ? s : k;  // (an empty run: nothing of mbuf s to decode)
    r.last_end = ends && run > 0 ? m0 + run : kNoBatch;
    r.pad_ = 0;
    *ws.cres = r;
    txn_begin[n_txn] = (uint32_t)n_acc;  // (n_txn <= max_txn, n_acc <= max_acc < 2^32)
    if (n_acc_dev) *n_acc_dev = (uint32_t)n_acc;
}

// the window's first n_emit mbufs, a wave each: lane m message m from the
// cursor (the last mbuf: below the plan's last_end) -- a CL_QRY's txn index a
// wave prefix over the CL_QRY flags, its boundary and reply fields; then all
// lanes the requests.  Everything lands behind the epoch's n_txn_in txns and
// n_acc_in accesses.
__global__ __launch_bounds__(kBlock) void k_wire_emit_calvin(dv_wire_cfg cfg, const uint8_t *__restrict__ buf,
                                                             const uint64_t *__restrict__ off, uint32_t first,
                                                             uint32_t msg0, dv_wire_dev_out out, uint32_t n_txn_in,
                                                             uint32_t n_acc_in, WireCalvinWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint32_t s_rq[kWireWave][64];
    __shared__ uint16_t s_p2[kWireWave][64], s_tx[kWireWave][64];  // message m's request count's offset, txns before it
    const uint32_t n_emit = ws.cres->n_emit;
    if (blockIdx.x * kWireWave >= n_emit) return;
    const WaveBatch w = stage_taken_batch(s_img, buf, off, first, n_emit);
    const uint32_t lane = w.lane, wave = w.wave, b = w.b;
    uint32_t src = 0, my_q = 0, my_n = 0, my_p2 = 0, t0 = 0, a0 = 0;
    uint64_t tid = 0, cst = 0;
    if (w.live) {
        src = w.st.u32(4);
        const uint32_t count = w.st.u32(8), last_end = b + 1 == n_emit ? ws.cres->last_end : kNoBatch;
        const uint32_t m0 = b == 0 ? msg0 : 0, mend = last_end < count ? last_end : count;
        batch_base(ws, b, t0, a0);
        t0 += n_txn_in;
        a0 += n_acc_in;
        if (lane >= m0 && lane < mend) {
            const uint32_t mo = ws.moff[(uint64_t)b * Calvin::kStride + lane];
            if (w.st.u32(mo) == DV_WIRE_CL_QRY) {
                my_q = 1;
                tid = w.st.u64(mo + kCalTxnId);  // the sequencer's
                query_fields<Calvin>(w.st, mo, cst, my_p2, my_n);
            }
        }
    }
    const uint32_t rq_in = wave_incl_sum(my_n, lane), q_in = wave_incl_sum(my_q, lane);
    const uint32_t tot_rq = __shfl(rq_in, 63, 64);
    s_rq[wave][lane] = rq_in - my_n;
    s_p2[wave][lane] = (uint16_t)my_p2;
    s_tx[wave][lane] = (uint16_t)(q_in - my_q);
    __syncthreads();
    if (!w.live) return;
    if (my_q) emit_txn_fields(out, t0 + q_in - 1u, a0 + rq_in - my_n, tid, cst, src);
    const uint16_t *tx = s_tx[wave];
    emit_requests(w.st, s_rq[wave], s_p2[wave], tot_rq, t0, a0, out, cfg.part_cnt, lane,
                  [tx](uint32_t m) { return (uint32_t)tx[m]; });
}

// the check, the scan and the plan of a sequencer stream's mbufs, `check` launched with the kernel's own arguments
template <class Check>
static void launch_stream_plan(hipStream_t s, uint32_t nb, uint32_t n_batches, uint32_t max_txn, uint64_t max_acc,
                               uint32_t *txn_begin, uint32_t *n_acc_dev, const dv_wire_calvin_pos &pos,
                               const WireCalvinWs &ws, Check check) {
    const uint32_t nc = (nb + kWireChunk - 1) / kWireChunk;
    (void)hipMemsetAsync(ws.first, 0xFF, 2 * sizeof(uint32_t), s);  // kNoBatch, both
    if (nb) {
        check((nb + kWireWave - 1) / kWireWave);
        DV_LAUNCH(k_wire_scan_calvin, nc, kBlock, 0, s, ws, nb, pos.batch_id);
    }
    DV_LAUNCH(k_wire_plan_calvin, 1, kBlock, 0, s, ws, nb, n_batches, nc, max_txn, max_acc, txn_begin, n_acc_dev, pos);
}

void launch_wire_plan_calvin(hipStream_t s, const dv_wire_cfg &cfg, const uint8_t *buf, uint64_t buf_len,
                             const uint64_t *off, uint32_t nb, uint32_t n_batches, const dv_wire_dev_out &out,
                             const dv_wire_calvin_pos &pos, const WireCalvinWs &ws) {
    launch_stream_plan(s, nb, n_batches, out.max_txn, out.max_acc, out.txn_begin, out.n_acc_dev, pos, ws,
                       [&](uint32_t grid) {
                           DV_LAUNCH(k_wire_check_calvin, grid, kBlock, 0, s, cfg, buf, buf_len, off, pos.batch,
                                     pos.msg, nb, ws);
                       });
}

void launch_wire_emit_calvin(hipStream_t s, const dv_wire_cfg &cfg, const uint8_t *buf, const uint64_t *off,
                             uint32_t nb, const dv_wire_dev_out &out, const dv_wire_calvin_pos &pos,
                             const WireCalvinWs &ws) {
    if (!nb) return;
    DV_LAUNCH(k_wire_emit_calvin, (nb + kWireWave - 1) / kWireWave, kBlock, 0, s, cfg, buf, off, pos.batch, pos.msg,
              out, pos.n_txn, (uint32_t)pos.n_acc, ws);
}

// ---- TPC-C under CALVIN (dv_wire_ingest_device_calvin_tpcc): the two
// dialects composed.  A CL_QRY is 207 + 8 np + 24 n bytes (Calvin::kFixed, the
// partitions, kTpccBody, the items, kTpccTail), an RDONE the header alone; the
// scan and the plan are the YCSB stream's as they are.
//
// dv_wire_open for a CALVIN TPC-C cfg, and a cursor below the count.  Lane m
// checks message m's fixed fields where it is a CL_QRY -- an RDONE lane reads
// no body byte: what lies behind its header is the next message, or nothing.
// Two prefix sums live side by side: the NewOrders' items of the whole mbuf,
// in the run or not (one flat range all lanes check: it is refused whole), and
// the accesses of the run alone, which keep_run sums.
__global__ __launch_bounds__(kBlock) void k_wire_check_calvin_tpcc(dv_wire_cfg cfg, dv_tpcc_params tp,
                                                                   const uint8_t *__restrict__ buf, uint64_t buf_len,
                                                                   const uint64_t *__restrict__ off, uint32_t first,
                                                                   uint32_t msg0, uint32_t nb, WireCalvinWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint32_t s_it[kWireWave][64], s_pp[kWireWave][64];  // items to check / partitions before message m
    __shared__ uint16_t s_mo[kWireWave][64], s_io[kWireWave][64];  // message m's offset, its first item's
    const WaveBatch w = stage_wave_batch(s_img, buf, buf_len, off, first, nb);
    const Stage &st = w.st;
    const uint32_t lane = w.lane, wave = w.wave;
    const uint32_t m0 = w.b == 0 ? msg0 : 0;  // the cursor's message (the window's first mbuf is the cursor's)
    const bool parse = w.live && !w.bad;
    bool bad = w.bad;
    uint32_t count = 0;
    Msg my{};
    if (parse)
        bad = !open_header<Calvin>(st, cfg, count) || m0 >= count ||
              !walk_chain<Calvin>(st, w.len, count, lane, my, [&](uint32_t bo, uint32_t &n) -> uint32_t {
                  return tpcc_body_end(st, w.len, bo, n);
              });
    bool wrong = false;
    uint32_t my_acc = 0, my_it = 0;
    if (parse && !bad && lane < count && my.rt == DV_WIRE_CL_QRY)
        wrong = tpcc_fields_wrong(st, tp, my.bo, my.n, my_acc, my_it);
    // (an RDONE's lane holds no partitions and no items: np = n = 0 from the walk)
    const uint32_t it_in = wave_incl_sum(my_it, lane), pp_in = wave_incl_sum(my.np, lane);
    const uint32_t tot_it = __shfl(it_in, 63, 64), tot_pp = __shfl(pp_in, 63, 64);
    s_it[wave][lane] = it_in - my_it;
    s_pp[wave][lane] = pp_in - my.np;
    s_mo[wave][lane] = (uint16_t)my.off;
    s_io[wave][lane] = (uint16_t)(my.bo + kTpccBody);
    __syncthreads();
    if (parse && !bad) {
        wrong |= parts_wrong<Calvin>(st, s_pp[wave], s_mo[wave], tot_pp, cfg.part_cnt, lane);
        wrong |= tpcc_items_wrong(st, tp, s_it[wave], s_io[wave], tot_it, lane);
    }
    bad = bad || __any(wrong);
    keep_run(ws, w, bad, count, m0, my, my_acc);  // (a txn is at most 3 + 2 * 62 accesses: the per-mbuf byte)
}

// the window's first n_emit mbufs, a wave each: lane m message m from the
// cursor (the last mbuf: below the plan's last_end) -- a CL_QRY's txn index a
// wave prefix over the CL_QRY flags, its boundary, txn type and reply fields,
// its lead left in LDS; then all lanes the run's accesses (k_wire_emit_tpcc's
// closed form), behind the epoch's n_txn_in txns and n_acc_in accesses
__global__ __launch_bounds__(kBlock) void k_wire_emit_calvin_tpcc(dv_wire_cfg cfg, dv_tpcc_params tp,
                                                                  const uint8_t *__restrict__ buf,
                                                                  const uint64_t *__restrict__ off, uint32_t first,
                                                                  uint32_t msg0, dv_wire_tpcc_dev_out out,
                                                                  uint32_t n_txn_in, uint32_t n_acc_in,
                                                                  WireCalvinWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint64_t s_hk[kWireWave][64][3], s_h[kWireWave][64];  // message m's leading keys, its h_amount
    __shared__ uint32_t s_ac[kWireWave][64], s_mt[kWireWave][64];    // accesses before message m, TpccLead::mt
    __shared__ uint16_t s_io[kWireWave][64], s_tx[kWireWave][64];    // message m's first item, txns before it
    const uint32_t n_emit = ws.cres->n_emit;
    if (blockIdx.x * kWireWave >= n_emit) return;
    const WaveBatch w = stage_taken_batch(s_img, buf, off, first, n_emit);
    const Stage &st = w.st;
    const uint32_t lane = w.lane, wave = w.wave, b = w.b;
    uint32_t src = 0, my_q = 0, t0 = 0, a0 = 0;
    uint64_t tid = 0, cst = 0;
    TpccLead my{};
    if (w.live) {
        src = st.u32(4);
        const uint32_t count = st.u32(8), last_end = b + 1 == n_emit ? ws.cres->last_end : kNoBatch;
        const uint32_t m0 = b == 0 ? msg0 : 0, mend = last_end < count ? last_end : count;
        batch_base(ws, b, t0, a0);
        t0 += n_txn_in;
        a0 += n_acc_in;
        if (lane >= m0 && lane < mend) {
            const uint32_t mo = ws.moff[(uint64_t)b * Calvin::kStride + lane];
            if (st.u32(mo) == DV_WIRE_CL_QRY) {
                my_q = 1;
                tid = st.u64(mo + kCalTxnId);  // the sequencer's
                cst = st.u64(mo + Calvin::kHdr);
                my = tpcc_lead(st, tp, mo + Calvin::kFixed + st.u32(mo + Calvin::kHdr + 8) * 8u);
            }
        }
    }
    const uint32_t ac_in = wave_incl_sum(my.acc, lane), q_in = wave_incl_sum(my_q, lane);
    const uint32_t tot_ac = __shfl(ac_in, 63, 64);
    const TpccLds t{s_hk[wave], s_h[wave], s_ac[wave], s_mt[wave], s_io[wave]};
    t.keep(lane, my, ac_in - my.acc);
    s_tx[wave][lane] = (uint16_t)(q_in - my_q);
    __syncthreads();
    if (!w.live) return;
    if (my_q) {
        const uint32_t txn = t0 + q_in - 1u;
        if (out.txn_type) out.txn_type[txn] = (uint8_t)my.tt;
        emit_txn_fields(out, txn, a0 + ac_in - my.acc, tid, cst, src);
    }
    const uint16_t *tx = s_tx[wave];
    emit_tpcc_accesses(st, tp, t, tot_ac, t0, a0, out, lane, [tx](uint32_t m) { return (uint32_t)tx[m]; });
}

void launch_wire_plan_calvin_tpcc(hipStream_t s, const dv_wire_cfg &cfg, const dv_tpcc_params &tp, const uint8_t *buf,
                                  uint64_t buf_len, const uint64_t *off, uint32_t nb, uint32_t n_batches,
                                  const dv_wire_tpcc_dev_out &out, const dv_wire_calvin_pos &pos,
                                  const WireCalvinWs &ws) {
    launch_stream_plan(s, nb, n_batches, out.max_txn, out.max_acc, out.txn_begin, out.n_acc_dev, pos, ws,
                       [&](uint32_t grid) {
                           DV_LAUNCH(k_wire_check_calvin_tpcc, grid, kBlock, 0, s, without_tpcc(cfg), tp, buf, buf_len,
                                     off, pos.batch, pos.msg, nb, ws);
                       });
}

void launch_wire_emit_calvin_tpcc(hipStream_t s, const dv_wire_cfg &cfg, const dv_tpcc_params &tp, const uint8_t *buf,
                                  const uint64_t *off, uint32_t nb, const dv_wire_tpcc_dev_out &out,
                                  const dv_wire_calvin_pos &pos, const WireCalvinWs &ws) {
    if (!nb) return;
    DV_LAUNCH(k_wire_emit_calvin_tpcc, (nb + kWireWave - 1) / kWireWave, kBlock, 0, s, without_tpcc(cfg), tp, buf, off,
              pos.batch, pos.msg, out, pos.n_txn, (uint32_t)pos.n_acc, ws);
}

// ---- the committed txns' reply fields, compacted in txn order
__global__ __launch_bounds__(kBlock) void k_reply_count(const uint8_t *__restrict__ commit, uint32_t n_txn,
                                                        uint32_t *__restrict__ bc) {
    __shared__ uint32_t lds4[4];
    const uint32_t t = blockIdx.x * kReplyTile + threadIdx.x;
    uint32_t tot = 0;
    (void)block_excl_scan256(t < n_txn && commit[t] ? 1u : 0u, lds4, &tot);
    if (threadIdx.x == 0) bc[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void k_reply_scan(uint32_t *__restrict__ bc, uint32_t nt) {
    __shared__ uint32_t lds4[4];
    const uint32_t tot = block_chunk_scan256(bc, nt, lds4);
    if (threadIdx.x == 0) bc[nt] = tot;
}

__global__ __launch_bounds__(kBlock) void k_reply_emit(const uint8_t *__restrict__ commit, uint32_t n_txn,
                                                       const uint32_t *__restrict__ bc,
                                                       const uint64_t *__restrict__ txn_id,
                                                       const uint64_t *__restrict__ cst,
                                                       const uint32_t *__restrict__ rnode,
                                                       uint64_t *__restrict__ o_txn_id, uint64_t *__restrict__ o_cst,
                                                       uint32_t *__restrict__ o_rnode) {
    __shared__ uint32_t lds4[4];
    const uint32_t t = blockIdx.x * kReplyTile + threadIdx.x;
    const bool cm = t < n_txn && commit[t];
    const uint32_t o = bc[blockIdx.x] + block_excl_scan256(cm ? 1u : 0u, lds4, nullptr);
    if (!cm) return;
    o_txn_id[o] = txn_id[t];
    o_cst[o] = cst[t];
    o_rnode[o] = rnode[t];
}

uint32_t reply_tiles(uint32_t n_txn) { return (n_txn + kReplyTile - 1) / kReplyTile; }

void launch_reply_fields(hipStream_t s, const uint8_t *commit, uint32_t n_txn, const uint64_t *txn_id,
                         const uint64_t *cst, const uint32_t *rnode, uint64_t *o_txn_id, uint64_t *o_cst,
                         uint32_t *o_rnode, uint32_t *bc) {
    const uint32_t nt = reply_tiles(n_txn);
    if (nt) DV_LAUNCH(k_reply_count, nt, kBlock, 0, s, commit, n_txn, bc);
    DV_LAUNCH(k_reply_scan, 1, kBlock, 0, s, bc, nt);
    if (nt) DV_LAUNCH(k_reply_emit, nt, kBlock, 0, s, commit, n_txn, bc, txn_id, cst, rnode, o_txn_id, o_cst, o_rnode);
}

// ---- the reply mbufs packed on the device (dv_wire_respond_device): what
// dv_wire_respond (csrc/wire.cpp) writes, from reply fields in device memory.
// A stable multi-split of the answered txns by destination, then a closed-form
// placement.  Per tile of kReplyTile txns the answered ones are counted per
// destination (k_rsp_count), each destination's tiles are scanned
// (k_rsp_scan), the destinations are scanned into their first mbuf and first
// message and the call is decided (k_rsp_plan); rank r of destination d is
// then message r % per of mbuf dmb[d] + r / per, and the dword it starts at is
//   3 * (dmb[d] + r / per + 1) + kDw * (dmsg[d] + r)
// -- every mbuf in front of it and its own carry a 12-byte header, every
// message in front of it is kDw dwords.  The emit (k_rsp_emit*) orders a
// tile's answered txns by (destination, rank) in LDS and walks their dwords
// with consecutive lanes on consecutive dwords: a destination's run is
// contiguous but for the headers, so a wave's store covers 256 contiguous
// bytes wherever a run is that long.  out is written in whole dwords (every
// size of the format is a multiple of 4 and out is 4-byte aligned), each once.
namespace {

static_assert(kBlock == DV_WIRE_DEST_MAX && kBlock == kReplyTile, "a thread per txn of the tile and per destination");

// A dialect's reply (ClientResponseMessage / AckMessage): kDw dwords -- rtype,
// txn_id, [batch_id,] 16 of mq_time and latencies, then client_startts or the
// ack's rc -- and kPer of them to a full mbuf.
struct RspClient {
    static constexpr uint32_t kDw = 21, kType = DV_WIRE_CL_RSP;
    static constexpr bool kCalvin = false, kSeq = false;
};
struct RspCalvin {
    static constexpr uint32_t kDw = 22, kType = DV_WIRE_CALVIN_ACK;
    static constexpr bool kCalvin = true, kSeq = false;
};
// a CALVIN sequencer's CL_RSP (dv_wire_sequence_acks_device): the CALVIN build's header, batch_id UINT64_MAX,
// then client_startts; the txn id is the sequencer's own, node_id + node_cnt * txn
struct RspSeq {
    static constexpr uint32_t kDw = 23, kType = DV_WIRE_CL_RSP;
    static constexpr bool kCalvin = false, kSeq = true;
};
template <class R>
constexpr uint32_t rsp_per() {
    return (DV_WIRE_MSG_MAX - DV_WIRE_HDR) / (R::kDw * 4);
}
static_assert(rsp_per<RspClient>() == 48 && rsp_per<RspCalvin>() == 46 && rsp_per<RspSeq>() == 44,
              "replies of a full mbuf");

// which entries of the call are answered, and by which txn's fields
struct RspSel {
    uint32_t n, n_src_txn;
    const uint8_t *commit;
    const uint32_t *src, *rnode;
    const uint32_t *n_dev;  // or NULL: the entries in use, where only the device knows them (at most n)
};

__device__ __forceinline__ bool rsp_answered(const RspSel &s, uint32_t i, uint32_t &txn) {
    txn = i;
    if (i >= s.n || (s.n_dev && i >= *s.n_dev)) return false;
    if (s.src) {
        txn = s.src[i];
        return true;
    }
    return !s.commit || s.commit[i] != 0;
}

// dword f of a reply
template <class R>
__device__ __forceinline__ uint32_t rsp_dword(uint32_t f, uint64_t txn_id, uint64_t tail) {
    // tail: CALVIN the batch id (dwords 3, 4; the rc behind the latencies is 0), else client_startts (the last two)
    constexpr uint32_t t0 = R::kCalvin ? 3 : R::kDw - 2;
    if (f == 0) return R::kType;
    if (f <= 2) return (uint32_t)(txn_id >> (32 * (f - 1)));
    if (R::kSeq && f <= 4) return 0xFFFFFFFFu;
    if (f == t0 || f == t0 + 1) return (uint32_t)(tail >> (32 * (f - t0)));
    return 0;
}

template <class R>
__device__ __forceinline__ void rsp_emit(const RspSel &sel, uint32_t nt, uint32_t node_id, uint64_t batch_id,
                                         const uint64_t *__restrict__ txn_id, const uint64_t *__restrict__ cst,
                                         const ReplyWs &ws, uint32_t *__restrict__ out,
                                         uint64_t *__restrict__ batch_off) {
    constexpr uint32_t per = rsp_per<R>();
    __shared__ uint32_t lds4[4], s_wave[4][DV_WIRE_DEST_MAX], s_first[DV_WIRE_DEST_MAX];
    __shared__ uint64_t s_pos[kReplyTile], s_id[kReplyTile], s_tail[kReplyTile];
    if (ws.res->status != DV_OK) return;  // (the plan refused the call: nothing is written)
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) s_wave[w][tid] = 0;
    __syncthreads();
    uint32_t txn;
    const bool ans = rsp_answered(sel, blockIdx.x * kReplyTile + tid, txn);
    const uint32_t d = ans ? sel.rnode[txn] : 0u;  // (< n_dest: the plan saw no err)
    // the txn's place among the wave's answered txns of its destination, then among the tile's
    const uint64_t peers = match_digit(d, __ballot(ans));
    const uint32_t in_wave = mask_rank(peers);
    if (ans && in_wave == 0) s_wave[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    uint32_t n_ans = 0;
    const uint32_t first = block_excl_scan256(s_wave[0][tid] + s_wave[1][tid] + s_wave[2][tid] + s_wave[3][tid], lds4,
                                              &n_ans);
    s_first[tid] = first;  // destination tid's first slot in the tile's (destination, rank) order
    __syncthreads();
    if (ans) {
        uint32_t in_tile = in_wave;
        for (uint32_t w = 0; w < wave; w++) in_tile += s_wave[w][d];
        const uint32_t r = ws.cnt[(uint64_t)d * nt + blockIdx.x] + in_tile;
        const uint32_t j = r / per, mb = ws.dmb[d] + j;
        const uint64_t pos = 3ull * ((uint64_t)mb + 1) + (uint64_t)R::kDw * ((uint64_t)ws.dmsg[d] + r);
        // (RspSeq: batch_id carries node_cnt)
        const uint64_t id = R::kSeq ? node_id + batch_id * txn : txn_id[txn], tail = R::kCalvin ? batch_id : cst[txn];
        if (r == j * per) {  // the mbuf's first message: its header and offset
            const uint32_t left = ws.tot[d] - r;
            out[pos - 3] = d;
            out[pos - 2] = node_id;
            out[pos - 1] = left < per ? left : per;
            batch_off[mb] = (pos - 3) * 4;
        }
#ifdef DVCC_RSP_EMIT_SIMPLE
        // the first form (A/B only): every thread its own message, a wave's stores kDw dwords apart
        for (uint32_t f = 0; f < R::kDw; f++) out[pos + f] = rsp_dword<R>(f, id, tail);
#else
        const uint32_t slot = s_first[d] + in_tile;
        s_pos[slot] = pos;
        s_id[slot] = id;
        s_tail[slot] = tail;
#endif
    }
#ifndef DVCC_RSP_EMIT_SIMPLE
    __syncthreads();
    for (uint32_t i = tid; i < n_ans * R::kDw; i += kBlock) {
        const uint32_t slot = i / R::kDw, f = i - slot * R::kDw;
        out[s_pos[slot] + f] = rsp_dword<R>(f, s_id[slot], s_tail[slot]);
    }
#endif
}

}  // namespace

// tile blockIdx.x: its answered txns per destination; a node or a list index out of range raises ws.err
__global__ __launch_bounds__(kBlock) void k_rsp_count(RspSel sel, uint32_t n_dest, uint32_t nt, ReplyWs ws) {
    __shared__ uint32_t s_cnt[DV_WIRE_DEST_MAX];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t txn;
    if (rsp_answered(sel, blockIdx.x * kReplyTile + threadIdx.x, txn)) {
        const uint32_t d = sel.src && txn >= sel.n_src_txn ? n_dest : sel.rnode[txn];
        if (d < n_dest) atomicAdd(&s_cnt[d], 1u);
        else atomicOr(ws.err, 1u);
    }
    __syncthreads();
    if (threadIdx.x < n_dest) ws.cnt[(uint64_t)threadIdx.x * nt + blockIdx.x] = s_cnt[threadIdx.x];
}

// destination blockIdx.x: its tiles' counts become the replies in front of each tile
__global__ __launch_bounds__(kBlock) void k_rsp_scan(ReplyWs ws, uint32_t nt) {
    __shared__ uint32_t lds4[4];
    const uint32_t tot = block_chunk_scan256(ws.cnt + (uint64_t)blockIdx.x * nt, nt, lds4);
    if (threadIdx.x == 0) ws.tot[blockIdx.x] = tot;
}

// One workgroup, a thread per destination: the mbufs and messages in front of
// each, the totals, and the call's fate -- decided here, before any byte of
// out or batch_off is written (the closing offset is this kernel's).
__global__ __launch_bounds__(kBlock) void k_rsp_plan(ReplyWs ws, uint32_t nt, uint32_t n_dest, uint32_t per,
                                                     uint32_t msg_bytes, uint64_t cap, uint32_t max_batches,
                                                     uint64_t *__restrict__ batch_off) {
    __shared__ uint32_t lds4[4];
    const uint32_t d = threadIdx.x;
    const uint32_t c = nt && d < n_dest ? ws.tot[d] : 0u;
    uint32_t tot_mb = 0, tot_msg = 0;
    const uint32_t mb = block_excl_scan256(c / per + (c % per ? 1u : 0u), lds4, &tot_mb);
    const uint32_t msg = block_excl_scan256(c, lds4, &tot_msg);
    if (d < n_dest) {
        ws.dmb[d] = mb;
        ws.dmsg[d] = msg;
    }
    if (d != 0) return;
    const bool bad = *ws.err != 0;
    const uint64_t bytes = (uint64_t)tot_mb * DV_WIRE_HDR + (uint64_t)tot_msg * msg_bytes;
    dv_wire_rsp_result r;
    r.status = bad || bytes > cap || tot_mb > max_batches ? DV_ERR_ARG : DV_OK;
    r.n_batches = bad ? 0u : tot_mb;
    r.n_msgs = bad ? 0u : tot_msg;
    r.pad_ = 0;
    r.n_bytes = bad ? 0ull : bytes;
    *ws.res = r;
    if (r.status == DV_OK) batch_off[tot_mb] = bytes;  // (tot_mb == 0: batch_off[0] = 0)
}

__global__ __launch_bounds__(kBlock) void k_rsp_emit(RspSel sel, uint32_t nt, uint32_t node_id,
                                                     const uint64_t *__restrict__ txn_id,
                                                     const uint64_t *__restrict__ cst, ReplyWs ws,
                                                     uint32_t *__restrict__ out, uint64_t *__restrict__ batch_off) {
    rsp_emit<RspClient>(sel, nt, node_id, 0, txn_id, cst, ws, out, batch_off);
}

__global__ __launch_bounds__(kBlock) void k_rsp_emit_calvin(RspSel sel, uint32_t nt, uint32_t node_id,
                                                            uint64_t batch_id, const uint64_t *__restrict__ txn_id,
                                                            ReplyWs ws, uint32_t *__restrict__ out,
                                                            uint64_t *__restrict__ batch_off) {
    rsp_emit<RspCalvin>(sel, nt, node_id, batch_id, txn_id, nullptr, ws, out, batch_off);
}

static RspSel rsp_sel(const dv_wire_rsp_in &in) {
    return RspSel{in.n, in.n_src_txn, in.commit, in.src, in.return_node, nullptr};
}

void launch_rsp_plan(hipStream_t s, const dv_wire_cfg &cfg, const dv_wire_rsp_in &in, const dv_wire_rsp_out &out,
                     const ReplyWs &ws) {
    const uint32_t nt = reply_tiles(in.n);
    const uint32_t per = cfg.calvin ? rsp_per<RspCalvin>() : rsp_per<RspClient>();
    const uint32_t msg_bytes = 4 * (cfg.calvin ? RspCalvin::kDw : RspClient::kDw);
    (void)hipMemsetAsync(ws.err, 0, sizeof(uint32_t), s);
    if (nt) {
        DV_LAUNCH(k_rsp_count, nt, kBlock, 0, s, rsp_sel(in), in.n_dest, nt, ws);
        DV_LAUNCH(k_rsp_scan, in.n_dest, kBlock, 0, s, ws, nt);
    }
    DV_LAUNCH(k_rsp_plan, 1, kBlock, 0, s, ws, nt, in.n_dest, per, msg_bytes, out.cap, out.max_batches, out.batch_off);
}

void launch_rsp_emit(hipStream_t s, const dv_wire_cfg &cfg, const dv_wire_rsp_in &in, const dv_wire_rsp_out &out,
                     const ReplyWs &ws) {
    const uint32_t nt = reply_tiles(in.n);
    if (!nt) return;
    uint32_t *out32 = reinterpret_cast<uint32_t *>(out.out);
    if (cfg.calvin)
        DV_LAUNCH(k_rsp_emit_calvin, nt, kBlock, 0, s, rsp_sel(in), nt, cfg.node_id, in.batch_id, in.txn_id, ws, out32,
                  out.batch_off);
    else
        DV_LAUNCH(k_rsp_emit, nt, kBlock, 0, s, rsp_sel(in), nt, cfg.node_id, in.txn_id, in.client_startts, ws, out32,
                  out.batch_off);
}

// ---- the CALVIN sequencer's batch out (dv_wire_sequence_device): what
// dv_wire_sequence (csrc/wire.cpp) writes.  Check, scan and plan as the
// ingests' -- a wave per client mbuf over a third dialect, Seq: a CALVIN
// build's 84-byte header on a client's CL_QRY, no RDONE -- then the new part,
// the cut.  A destination's messages (and its RDONE) are a list; an entry's
// bytes in front of it, S, come from per-(destination, mbuf) counts scanned per
// destination (k_seq_dscan) and a wave's own prefix (k_seq_list).  next(i), the
// first entry that no longer fits an mbuf opened at i, is a search on S, and
// the mbuf starts are the entries reachable from 0 along next.  They are
// resolved by pointer jumping inside tiles of kSeqTile entries in LDS
// (k_seq_tiles: from every entry, where the walk leaves the tile and the mbufs
// it opens on the way), one thread per destination chaining the tiles
// (k_seq_chain: where the walk enters each tile), and the tiles marking their
// starts from that entry by the jump levels (k_seq_marks), which also places
// every entry in out and writes the mbuf headers, the offsets and the RDONEs.
// The second plan (k_seq_plan2) decides bytes and mbufs against the capacities
// before any of that is written.  The emit (k_seq_emit) stages a taken mbuf
// again and copies each message once per participant, consecutive lanes on
// consecutive dwords of a message: every size is a multiple of 4 and out is
// 4-byte aligned, so out is written in whole dwords, each once.
namespace {

struct Seq {
    static constexpr uint32_t kHdr = 84, kFixed = 100, kStride = kWireMaxMsg;
    static constexpr bool kRdone = false;
};
constexpr uint32_t kSeqRoom = kWireMsgMax - DV_WIRE_HDR;  // message bytes of an mbuf
constexpr uint32_t kSeqHdrDw = Seq::kHdr / 4;

// lane d: where destination d's list starts (every lane of the wave calls)
__device__ __forceinline__ uint32_t seq_list_base(const uint32_t *__restrict__ dtot, uint32_t nodes, uint32_t lane) {
    const uint32_t v = lane < nodes ? dtot[lane] + 2u : 0u;
    return wave_incl_sum(v, lane) - v;
}

// s[i]: the bytes in front of entry r0 + i of a destination's list (tot
// messages of totb bytes, then the RDONE; behind the list's end: nothing fits),
// for a tile and the reach behind it.  Every thread of the block; a barrier.
__device__ __forceinline__ void seq_tile_sums(const uint32_t *__restrict__ lS, uint32_t tot, uint32_t totb, uint32_t r0,
                                              uint32_t *s) {
    for (uint32_t i = threadIdx.x; i < kSeqTile + kSeqReach; i += kBlock) {
        const uint32_t r = r0 + i;
        s[i] = r < tot ? lS[r] : (r == tot ? totb : (r == tot + 1 ? totb + Seq::kHdr : 0xFFFFFFFFu));
    }
    __syncthreads();
}

// the first entry that does not fit an mbuf opened at entry i (both tile-local): a message is 108 bytes at
// least and the RDONE 84, so it lies fewer than kSeqReach entries on
__device__ __forceinline__ uint32_t seq_next(const uint32_t *s, uint32_t i) {
    const uint32_t target = s[i] + kSeqRoom;
    uint32_t k = 0;
#pragma unroll
    for (uint32_t w = kSeqReach / 2; w > 0; w >>= 1)
        if (s[i + k + w] <= target) k += w;
    return i + k;
}

// ---- a TPC-C cfg's out: every size is 3 mod 4, so entries (mbuf headers,
// messages, RDONEs) start at any byte and neighbours share dwords, written by
// different threads, waves and kernels.  No dword is ever read back: a dword
// wholly inside one entry is one aligned dword store, the bytes at an entry's
// two edges are byte stores.  byte_at(k) / dword_at(k): the entry's byte k, its
// bytes [k, k + 4) -- composed per position in the entry, whatever its start.
// One thread writes the entry's n bytes at out's byte pos.
template <class ByteAt>
__device__ __forceinline__ void seq_put_entry(uint32_t *out, uint64_t pos, uint32_t n, ByteAt byte_at) {
    uint8_t *out8 = reinterpret_cast<uint8_t *>(out);
    uint32_t k = 0;
    for (; k < n && ((pos + k) & 3u); k++) out8[pos + k] = (uint8_t)byte_at(k);
    for (; k + 4 <= n; k += 4)
        out[(pos + k) >> 2] = byte_at(k) | byte_at(k + 1) << 8 | byte_at(k + 2) << 16 | byte_at(k + 3) << 24;
    for (; k < n; k++) out8[pos + k] = (uint8_t)byte_at(k);
}

// byte k of a stamped header: rtype, txn_id, batch_id, then mq_time and the latencies, zero
__device__ __forceinline__ uint32_t seq_hdr_byte(uint32_t k, uint32_t rtype, uint64_t id, uint64_t batch_id) {
    if (k < 4) return (rtype >> (8 * k)) & 0xFFu;
    if (k < 12) return (uint32_t)(id >> (8 * (k - 4))) & 0xFFu;
    if (k < 20) return (uint32_t)(batch_id >> (8 * (k - 12))) & 0xFFu;
    return 0;
}

// bytes [k, k + 4) of a stamped CL_QRY whose client bytes lie at o of the image
__device__ __forceinline__ uint32_t seq_msg_dword(const Stage &st, uint32_t o, uint32_t k, uint64_t id,
                                                  uint64_t batch_id) {
    if (k >= Seq::kHdr) return st.u32(o + k);
    if (k >= 20 && k + 4 <= Seq::kHdr) return 0;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t kk = k + j;
        const uint32_t by = kk < Seq::kHdr ? seq_hdr_byte(kk, DV_WIRE_CL_QRY, id, batch_id) : st.u32(o + kk) & 0xFFu;
        v |= by << (8 * j);
    }
    return v;
}

}  // namespace

__global__ __launch_bounds__(kBlock) void k_seq_check(dv_wire_cfg cfg, uint32_t n_dest,
                                                      const uint8_t *__restrict__ buf, uint64_t buf_len,
                                                      const uint64_t *__restrict__ off, uint32_t first, uint32_t nb,
                                                      WireSeqWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ YcsbTables s_t;
    __shared__ uint32_t s_pm[kWireWave][64][2];  // message m's participants
    __shared__ uint16_t s_sz[kWireWave][64];     // its bytes
    s_pm[threadIdx.x >> 6][threadIdx.x & 63][0] = 0;
    s_pm[threadIdx.x >> 6][threadIdx.x & 63][1] = 0;
    const WaveBatch w = stage_wave_batch(s_img, buf, buf_len, off, first, nb);
    const Stage &st = w.st;
    const uint32_t lane = w.lane, wave = w.wave;
    const bool parse = w.live && !w.bad;
    uint32_t count = 0, tot_rq = 0;
    Msg my{};
    bool bad = ycsb_batch_bad<Seq>(w, cfg, 0, s_t, count, my, tot_rq);
    if (parse && !bad) {  // ISCLIENTN(src); a txn has a request at least
        const uint32_t src = st.u32(4);
        bad = src < cfg.node_cnt || src >= n_dest;
    }
    bad = bad || __any(parse && lane < count && my.n == 0);
    if (parse && !bad)  // YCSBQuery::participants: GET_NODE_ID(key_to_part(key))
        for (uint32_t r = lane; r < tot_rq; r += 64) {
            const uint32_t m = last_le64(s_t.rq[wave], r);
            const uint64_t key = st.u64(s_t.p2[wave][m] + 8u + (r - s_t.rq[wave][m]) * kReqBytes + 8u);
            const uint32_t node = (uint32_t)((key % cfg.part_cnt) % cfg.node_cnt);
            atomicOr(&s_pm[wave][m][node >> 5], 1u << (node & 31u));
        }
    const uint32_t size = parse && !bad && lane < count ? my.bo + 8u + my.n * kReqBytes - my.off : 0u;
    s_sz[wave][lane] = (uint16_t)size;
    __syncthreads();
    const uint64_t mask = parse && !bad && lane < count ? ((uint64_t)s_pm[wave][lane][1] << 32) | s_pm[wave][lane][0] : 0;
    const uint32_t sends = __shfl(wave_incl_sum((uint32_t)__popcll(mask), lane), 63, 64);
    if (!w.live) return;
    keep_batch<Seq>(ws, w, bad, count, my.off, count, sends, count);  // (bm: the mbuf's messages)
    if (!bad && lane < count) {
        ws.mmask[(uint64_t)w.b * Seq::kStride + lane] = mask;
        ws.msz[(uint64_t)w.b * Seq::kStride + lane] = (uint16_t)size;
    }
    if (lane < cfg.node_cnt) {  // destination `lane`: its messages and bytes of this mbuf
        uint32_t c = 0, by = 0;
        for (uint32_t m = 0; !bad && m < count; m++)
            if (s_pm[wave][m][lane >> 5] >> (lane & 31u) & 1u) c++, by += s_sz[wave][m];
        ws.dcnt[(uint64_t)lane * nb + w.b] = c;
        ws.dbyt[(uint64_t)lane * nb + w.b] = by;
    }
}

// The same for a TPC-C cfg: k_wire_check_tpcc's checks over the Seq dialect
// (a CALVIN-build TPCCClientQueryMessage is 207 + 8 np + 24 n bytes, always
// 3 mod 4), then TPCCQuery::participants (tpcc_query.cpp:67-90): lane m adds
// the nodes of message m's w_id and, for a Payment, c_w_id; the mbuf's
// NewOrder items, one flat range, add their supply warehouses' -- a Payment's
// items are not in that range, they never add a participant.
static_assert(Seq::kFixed + kTpccBody + kTpccTail == 207 && 207 >= Seq::kHdr,
              "the smallest message is no shorter than the RDONE: kSeqReach holds as for YCSB");
static_assert((kSeqRoom / 207 + 1) <= kSeqReach && kSeqRoom / 207 == 19 && 19 <= kWireMaxMsg,
              "an mbuf holds at most 19 TPC-C messages");
// an mbuf's participants: a message of n items names 1 + n nodes at most (a
// Payment 2 in 207 bytes), so at most (1 + n) / (207 + 24 n) per byte, largest at n = 62
static_assert((uint64_t)kSeqRoom * (1 + DV_TPCC_MAX_OL) / (207 + 24 * DV_TPCC_MAX_OL) == 151 &&
                  kSeqRoom * 2 / 207 <= 151 && 151 <= kSeqMbufParts,
              "wire_seq_list_cap's bound per mbuf holds for TPC-C");
__global__ __launch_bounds__(kBlock) void k_seq_check_tpcc(dv_wire_cfg cfg, dv_tpcc_params tp, uint32_t n_dest,
                                                           const uint8_t *__restrict__ buf, uint64_t buf_len,
                                                           const uint64_t *__restrict__ off, uint32_t first,
                                                           uint32_t nb, WireSeqWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint32_t s_it[kWireWave][64], s_pp[kWireWave][64];  // NewOrder items / partitions before message m
    __shared__ uint16_t s_mo[kWireWave][64], s_io[kWireWave][64];  // message m's offset, its first item's
    __shared__ uint32_t s_pm[kWireWave][64][2];                    // message m's participants
    __shared__ uint16_t s_sz[kWireWave][64];                       // its bytes
    s_pm[threadIdx.x >> 6][threadIdx.x & 63][0] = 0;
    s_pm[threadIdx.x >> 6][threadIdx.x & 63][1] = 0;
    const WaveBatch w = stage_wave_batch(s_img, buf, buf_len, off, first, nb);
    const Stage &st = w.st;
    const uint32_t lane = w.lane, wave = w.wave;
    const bool parse = w.live && !w.bad;
    bool bad = w.bad;
    uint32_t count = 0;
    Msg my{};
    if (parse) {
        const uint32_t src = st.u32(4);  // ISCLIENTN(src)
        bad = !open_header<Seq>(st, cfg, count) || src < cfg.node_cnt || src >= n_dest ||
              !walk_chain<Seq>(st, w.len, count, lane, my, [&](uint32_t bo, uint32_t &n) -> uint32_t {
                  return tpcc_body_end(st, w.len, bo, n);
              });
    }
    bool wrong = false;
    uint32_t my_acc = 0, my_it = 0;
    if (parse && !bad && lane < count) wrong = tpcc_fields_wrong(st, tp, my.bo, my.n, my_acc, my_it);
    // (a bad mbuf's lanes hold zeros or a part of the chain: its tables are not read)
    const uint32_t it_in = wave_incl_sum(my_it, lane), pp_in = wave_incl_sum(my.np, lane);
    const uint32_t tot_it = __shfl(it_in, 63, 64), tot_pp = __shfl(pp_in, 63, 64);
    s_it[wave][lane] = it_in - my_it;
    s_pp[wave][lane] = pp_in - my.np;
    s_mo[wave][lane] = (uint16_t)my.off;
    s_io[wave][lane] = (uint16_t)(my.bo + kTpccBody);
    __syncthreads();
    if (parse && !bad) {
        wrong |= parts_wrong<Seq>(st, s_pp[wave], s_mo[wave], tot_pp, cfg.part_cnt, lane);
        wrong |= tpcc_items_wrong(st, tp, s_it[wave], s_io[wave], tot_it, lane);
    }
    bad = bad || __any(wrong);
    const bool good = parse && !bad;
    if (good) {  // (checked: every warehouse is in [1, num_wh], a 32-bit value)
        const auto add = [&](uint32_t m, uint32_t wh) {
            const uint32_t node = ((wh - 1) % tp.part_cnt) % cfg.node_cnt;
            atomicOr(&s_pm[wave][m][node >> 5], 1u << (node & 31u));
        };
        if (lane < count) {
            add(lane, st.u32(my.bo + 8));
            if (st.u32(my.bo) == 1) add(lane, st.u32(my.bo + 40));
        }
        for (uint32_t q = lane; q < tot_it; q += 64) {
            const uint32_t m = last_le64(s_it[wave], q);
            add(m, st.u32(s_io[wave][m] + (q - s_it[wave][m]) * kItemBytes + 8u));
        }
    }
    const uint32_t size = good && lane < count ? my.bo + kTpccBody + my.n * kItemBytes + kTpccTail - my.off : 0u;
    s_sz[wave][lane] = (uint16_t)size;
    __syncthreads();
    const uint64_t mask = good && lane < count ? ((uint64_t)s_pm[wave][lane][1] << 32) | s_pm[wave][lane][0] : 0;
    const uint32_t sends = __shfl(wave_incl_sum((uint32_t)__popcll(mask), lane), 63, 64);
    if (!w.live) return;
    keep_batch<Seq>(ws, w, bad, count, my.off, count, sends, count);  // (bm: the mbuf's messages)
    if (!bad && lane < count) {
        ws.mmask[(uint64_t)w.b * Seq::kStride + lane] = mask;
        ws.msz[(uint64_t)w.b * Seq::kStride + lane] = (uint16_t)size;
    }
    if (lane < cfg.node_cnt) {  // destination `lane`: its messages and bytes of this mbuf
        uint32_t c = 0, by = 0;
        for (uint32_t m = 0; !bad && m < count; m++)
            if (s_pm[wave][m][lane >> 5] >> (lane & 31u) & 1u) c++, by += s_sz[wave][m];
        ws.dcnt[(uint64_t)lane * nb + w.b] = c;
        ws.dbyt[(uint64_t)lane * nb + w.b] = by;
    }
}

// One workgroup: k_wire_plan's cut over the txns alone
__global__ __launch_bounds__(kBlock) void k_seq_plan(WireSeqWs ws, uint32_t first, uint32_t nb, uint32_t n_batches,
                                                     uint32_t nc, uint32_t max_txn) {
    __shared__ uint32_t lds4[4], s_chunk, s_cut;
    if (threadIdx.x == 0) {
        s_chunk = nc;
        s_cut = nb;
    }
    const uint32_t tot_t = block_chunk_scan256(ws.ct, nc, lds4);
    const uint32_t tot_a = block_chunk_scan256(ws.ca, nc, lds4);
    __syncthreads();
    const uint32_t cut = first_overflow(ws, nb, nc, tot_t, tot_a, max_txn, ~0ull, &s_chunk, &s_cut);
    const uint32_t fb = ws.first[0];
    const uint32_t k = fb < cut ? fb : cut;
    if (threadIdx.x != 0) return;
    WireSeqPlan p{};
    p.taken = k;
    p.n_txn = sum_below(ws.ct, ws.bt, k, nb, tot_t);
    p.n_msgs = sum_below(ws.ca, ws.ba, k, nb, tot_a);
    p.status = DV_OK;
    if (fb < nb && fb <= cut) p.status = DV_ERR_ARG;
    else if (cut < nb) p.status = cut ? DV_WIRE_MORE : DV_ERR_ARG;
    else if (first + nb < n_batches) p.status = DV_WIRE_MORE;
    *ws.plan = p;
}

// destination blockIdx.x: its counts per taken mbuf become those in front of the mbuf
__global__ __launch_bounds__(kBlock) void k_seq_dscan(WireSeqWs ws, uint32_t nb) {
    __shared__ uint32_t lds4[4];
    const uint32_t taken = ws.plan->taken;
    const uint32_t c = block_chunk_scan256(ws.dcnt + (uint64_t)blockIdx.x * nb, taken, lds4);
    const uint32_t by = block_chunk_scan256(ws.dbyt + (uint64_t)blockIdx.x * nb, taken, lds4);
    if (threadIdx.x == 0) {
        ws.dtot[blockIdx.x] = c;
        ws.dtotb[blockIdx.x] = by;
    }
}

// a wave per taken mbuf: every (message, participant) its list entry's S
__global__ __launch_bounds__(kBlock) void k_seq_list(WireSeqWs ws, uint32_t nb, uint32_t nodes) {
    const uint32_t lane = threadIdx.x & 63, b = blockIdx.x * kWireWave + (threadIdx.x >> 6);
    if (b >= ws.plan->taken) return;  // (the whole wave)
    const uint32_t lb = seq_list_base(ws.dtot, nodes, lane);
    const uint32_t count = ws.bm[b];
    const uint64_t mask = lane < count ? ws.mmask[(uint64_t)b * Seq::kStride + lane] : 0;
    const uint32_t size = lane < count ? ws.msz[(uint64_t)b * Seq::kStride + lane] : 0u;
    for (uint32_t d = 0; d < nodes; d++) {
        const bool has = mask >> d & 1u;
        const uint64_t bal = __ballot(has);
        if (!bal) continue;
        const uint32_t mine = has ? size : 0u, pre = wave_incl_sum(mine, lane) - mine;
        const uint32_t e = __shfl(lb, (int)d, 64) + ws.dcnt[(uint64_t)d * nb + b] + mask_rank(bal);
        if (has) ws.lS[e] = ws.dbyt[(uint64_t)d * nb + b] + pre;
    }
}

// tile blockIdx.x of destination blockIdx.y: from every entry, the walk along next inside the tile
__global__ __launch_bounds__(kBlock) void k_seq_tiles(WireSeqWs ws, uint32_t nodes) {
    __shared__ uint32_t s_S[kSeqTile + kSeqReach];
    __shared__ uint16_t s_p[kSeqTile], s_c[kSeqTile];
    static_assert(kSeqTile == kBlock, "a thread per entry");
    const uint32_t d = blockIdx.y, r0 = blockIdx.x * kSeqTile, tot = ws.dtot[d], L = tot + 1, i = threadIdx.x;
    if (r0 >= L) return;  // (the whole block)
    const uint32_t lb = __shfl(seq_list_base(ws.dtot, nodes, i & 63), (int)d, 64);
    seq_tile_sums(ws.lS + lb, tot, ws.dtotb[d], r0, s_S);
    const bool valid = r0 + i < L;
    uint32_t p = valid ? seq_next(s_S, i) : kSeqTile, c = valid ? 1u : 0u;  // (behind the list: out at once, no mbuf)
    s_p[i] = (uint16_t)p;
    s_c[i] = (uint16_t)c;
    __syncthreads();
#pragma unroll 1
    for (uint32_t round = 0; round < 8; round++) {  // (2^8 = kSeqTile steps at most)
        uint32_t np = p, ac = 0;
        if (p < kSeqTile) {
            np = s_p[p];
            ac = s_c[p];
        }
        __syncthreads();
        p = np;
        c += ac;
        s_p[i] = (uint16_t)p;
        s_c[i] = (uint16_t)c;
        __syncthreads();
    }
    if (valid) ws.ljmp[lb + r0 + i] = c << 8 | (p - kSeqTile);
}

// destination blockIdx.x, one thread: the walk from entry 0 from tile to tile
__global__ __launch_bounds__(64) void k_seq_chain(WireSeqWs ws, uint32_t nodes, uint32_t ntile) {
    const uint32_t d = blockIdx.x, lane = threadIdx.x;
    const uint32_t lb = __shfl(seq_list_base(ws.dtot, nodes, lane), (int)d, 64), L = ws.dtot[d] + 1;
    if (lane != 0) return;
    uint32_t x = 0, mbs = 0, t_next = 0;
    while (x < L) {
        const uint32_t t = x / kSeqTile, j = ws.ljmp[lb + x];
        ws.tent[(uint64_t)d * ntile + t] = x % kSeqTile;
        ws.tmb[(uint64_t)d * ntile + t] = mbs;
        mbs += j >> 8;
        x = (t + 1) * kSeqTile + (j & 255u);
        t_next = t + 1;
    }
    // (the last mbuf may reach over the list's last tile: the walk never enters it, no entry of it is a start)
    for (uint32_t t = t_next; t * kSeqTile < L; t++) {
        ws.tent[(uint64_t)d * ntile + t] = kNoBatch;
        ws.tmb[(uint64_t)d * ntile + t] = mbs;
    }
    ws.dmb[d] = mbs;
}

// one thread: the destinations' first mbufs and bytes, and the call's fate -- before any output is written
__global__ __launch_bounds__(64) void k_seq_plan2(WireSeqWs ws, uint32_t nodes, uint32_t first, uint64_t cap,
                                                  uint32_t max_batches) {
    if (threadIdx.x != 0) return;
    uint32_t mb = 0;
    uint64_t by = 0;
    for (uint32_t d = 0; d < nodes; d++) {
        ws.dMB[d] = mb;
        ws.dDB[d] = by;
        mb += ws.dmb[d];
        by += (uint64_t)ws.dtotb[d] + Seq::kHdr + (uint64_t)DV_WIRE_HDR * ws.dmb[d];
    }
    const WireSeqPlan p = *ws.plan;
    const bool refused = by > cap || mb > max_batches;
    ws.plan->refused = refused ? 1u : 0u;
    dv_wire_seq_result r;
    r.status = refused ? DV_ERR_ARG : p.status;
    r.n_taken = first + p.taken;
    r.n_txn = p.n_txn;
    r.n_out = mb;
    r.n_msgs = p.n_msgs;
    r.n_bytes = by;
    *ws.sres = r;
}

// the tiles again: the starts reachable from where the walk enters the tile,
// every entry's byte in out, the mbufs' headers and offsets, the RDONE.
// kBytes: a TPC-C cfg's byte-granular out (seq_put_entry); YCSB's whole dwords otherwise.
template <bool kBytes>
__device__ __forceinline__ void seq_marks(const WireSeqWs &ws, uint32_t nodes, uint32_t ntile, uint32_t node_id,
                                          uint64_t batch_id, uint32_t *__restrict__ out,
                                          uint64_t *__restrict__ batch_off, uint32_t *__restrict__ dest_first) {
    __shared__ uint32_t s_S[kSeqTile + kSeqReach], s_mark[kSeqTile], lds4[4];
    __shared__ uint16_t s_lv[8][kSeqTile];  // level k: 2^k steps along next, kSeqTile: out of the tile
    if (ws.plan->refused) return;
    const uint32_t d = blockIdx.y, r0 = blockIdx.x * kSeqTile, tot = ws.dtot[d], L = tot + 1, i = threadIdx.x;
    if (r0 >= L) return;  // (the whole block)
    const uint32_t lb = __shfl(seq_list_base(ws.dtot, nodes, i & 63), (int)d, 64);
    seq_tile_sums(ws.lS + lb, tot, ws.dtotb[d], r0, s_S);
    const uint32_t r = r0 + i;
    const bool valid = r < L;
    const uint32_t nxt = valid ? seq_next(s_S, i) : kSeqTile;
    s_lv[0][i] = (uint16_t)(nxt < kSeqTile ? nxt : kSeqTile);
    s_mark[i] = i == ws.tent[(uint64_t)d * ntile + blockIdx.x] ? 1u : 0u;
    __syncthreads();
    for (uint32_t k = 1; k < 8; k++) {
        const uint32_t v = s_lv[k - 1][i];
        s_lv[k][i] = v < kSeqTile ? s_lv[k - 1][v] : (uint16_t)kSeqTile;
        __syncthreads();
    }
    // (a mark set and followed inside one level is a step along next all the same: only entries of the walk are marked)
    for (int k = 7; k >= 0; k--) {
        const uint32_t v = s_lv[k][i];
        if (s_mark[i] && v < kSeqTile) s_mark[v] = 1u;
        __syncthreads();
    }
    const bool start = valid && s_mark[i] != 0;  // (the list's end may be marked: no entry)
    const uint32_t before = block_excl_scan256(start ? 1u : 0u, lds4, nullptr);
    if (valid) {
        const uint32_t j = ws.tmb[(uint64_t)d * ntile + blockIdx.x] + before + (start ? 1u : 0u) - 1u;  // its mbuf
        const uint64_t pos = ws.dDB[d] + (uint64_t)DV_WIRE_HDR * (j + 1) + s_S[i], q = pos >> 2;
        ws.lpos[lb + r] = pos;
        if (start && j < ws.dmb[d]) {  // (always: the chain counted the same starts)
            if constexpr (kBytes) {
                const uint32_t h[3] = {d, node_id, nxt - i};
                seq_put_entry(out, pos - DV_WIRE_HDR, DV_WIRE_HDR,
                              [&](uint32_t k) { return (h[k >> 2] >> (8 * (k & 3u))) & 0xFFu; });
            } else {
                out[q - 3] = d;
                out[q - 2] = node_id;
                out[q - 1] = nxt - i;
            }
            batch_off[ws.dMB[d] + j] = pos - DV_WIRE_HDR;
        }
        if (r == tot && pos + Seq::kHdr <= ws.sres->n_bytes) {  // the RDONE: the header alone (the bound: always)
            if constexpr (kBytes) {
                seq_put_entry(out, pos, Seq::kHdr,
                              [&](uint32_t k) { return seq_hdr_byte(k, DV_WIRE_RDONE, kNoBatchId, batch_id); });
            } else {
                out[q] = DV_WIRE_RDONE;
                out[q + 1] = out[q + 2] = 0xFFFFFFFFu;
                out[q + 3] = (uint32_t)batch_id;
                out[q + 4] = (uint32_t)(batch_id >> 32);
                for (uint32_t f = 5; f < kSeqHdrDw; f++) out[q + f] = 0;
            }
        }
    }
    if (blockIdx.x == 0 && i == 0) {
        dest_first[d] = ws.dMB[d];
        if (d == 0) {
            dest_first[nodes] = ws.sres->n_out;
            batch_off[ws.sres->n_out] = ws.sres->n_bytes;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_seq_marks(WireSeqWs ws, uint32_t nodes, uint32_t ntile, uint32_t node_id,
                                                      uint64_t batch_id, uint32_t *__restrict__ out,
                                                      uint64_t *__restrict__ batch_off,
                                                      uint32_t *__restrict__ dest_first) {
    seq_marks<false>(ws, nodes, ntile, node_id, batch_id, out, batch_off, dest_first);
}
__global__ __launch_bounds__(kBlock) void k_seq_marks_bytes(WireSeqWs ws, uint32_t nodes, uint32_t ntile,
                                                            uint32_t node_id, uint64_t batch_id,
                                                            uint32_t *__restrict__ out,
                                                            uint64_t *__restrict__ batch_off,
                                                            uint32_t *__restrict__ dest_first) {
    seq_marks<true>(ws, nodes, ntile, node_id, batch_id, out, batch_off, dest_first);
}

// the taken mbufs, a wave each: the wait list, and every message once per participant.
// kBytes: a message starts at any byte of out -- lanes 0..2 its bytes up to the
// first aligned dword and behind the last, consecutive lanes the dwords between.
template <bool kBytes>
__device__ __forceinline__ void seq_emit(const dv_wire_cfg &cfg, const uint8_t *__restrict__ buf,
                                         const uint64_t *__restrict__ off, uint32_t first, uint32_t nb,
                                         uint64_t batch_id, const WireSeqWs &ws, uint32_t *__restrict__ out,
                                         uint32_t *__restrict__ wait_client, uint64_t *__restrict__ wait_startts,
                                         uint32_t *__restrict__ wait_acks) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    const uint32_t taken = ws.plan->taken;
    if (ws.plan->refused || blockIdx.x * kWireWave >= taken) return;
    const WaveBatch w = stage_taken_batch(s_img, buf, off, first, taken);
    const Stage &st = w.st;
    const uint32_t lane = w.lane;
    const uint32_t lb = seq_list_base(ws.dtot, cfg.node_cnt, lane);
    if (!w.live) return;
    const uint32_t b = w.b, count = ws.bm[b], t0 = ws.ct[b / kWireChunk] + ws.bt[b];
    const uint64_t n_bytes = ws.sres->n_bytes;
    const uint64_t end = n_bytes >> 2;  // (no store at or past it, whatever the words above hold)
    uint64_t mask = 0;
    uint32_t size = 0, mo = 0;
    if (lane < count) {
        mo = ws.moff[(uint64_t)b * Seq::kStride + lane];
        mask = ws.mmask[(uint64_t)b * Seq::kStride + lane];
        size = ws.msz[(uint64_t)b * Seq::kStride + lane];
        wait_client[t0 + lane] = st.u32(4);
        wait_startts[t0 + lane] = st.u64(mo + Seq::kHdr);
        wait_acks[t0 + lane] = (uint32_t)__popcll(mask);
    }
    for (uint32_t d = 0; d < cfg.node_cnt; d++) {
        const bool has = mask >> d & 1u;
        uint64_t bal = __ballot(has);
        if (!bal) continue;
        const uint32_t e = __shfl(lb, (int)d, 64) + ws.dcnt[(uint64_t)d * nb + b] + mask_rank(bal);
        const uint64_t pos = has ? ws.lpos[e] : 0;
        while (bal) {  // the messages to d, one after the other: consecutive lanes, consecutive dwords
            const uint32_t m = (uint32_t)__builtin_ctzll(bal);
            bal &= bal - 1;
            const uint64_t id = worker_txn_id(cfg, t0 + m);
            if constexpr (kBytes) {
                const uint64_t p = shfl_u64(pos, m);
                const uint32_t o = __shfl(mo, (int)m, 64), sz = __shfl(size, (int)m, 64);
                const uint32_t head = (4u - (uint32_t)(p & 3u)) & 3u, ndw = (sz - head) >> 2;  // (sz >= 207)
                const uint32_t tail0 = head + 4u * ndw;
                uint8_t *out8 = reinterpret_cast<uint8_t *>(out);
                if (lane < head && p + lane < n_bytes)
                    out8[p + lane] = (uint8_t)seq_msg_dword(st, o, lane, id, batch_id);
                if (tail0 + lane < sz && p + tail0 + lane < n_bytes)
                    out8[p + tail0 + lane] = (uint8_t)seq_msg_dword(st, o, tail0 + lane, id, batch_id);
                for (uint32_t f = lane; f < ndw && p + head + 4u * f + 4u <= n_bytes; f += 64)
                    out[(p + head + 4u * f) >> 2] = seq_msg_dword(st, o, head + 4u * f, id, batch_id);
                continue;
            }
            const uint64_t q = shfl_u64(pos, m) >> 2;
            const uint32_t o = __shfl(mo, (int)m, 64), ndw = __shfl(size, (int)m, 64) >> 2;
            for (uint32_t f = lane; f < ndw && q + f < end; f += 64) {
                uint32_t v = 0;  // mq_time, the latencies
                if (f == 0) v = DV_WIRE_CL_QRY;
                else if (f <= 2) v = (uint32_t)(id >> (32 * (f - 1)));
                else if (f <= 4) v = (uint32_t)(batch_id >> (32 * (f - 3)));
                else if (f >= kSeqHdrDw) v = st.u32(o + 4 * f);
                out[q + f] = v;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_seq_emit(dv_wire_cfg cfg, const uint8_t *__restrict__ buf,
                                                     const uint64_t *__restrict__ off, uint32_t first, uint32_t nb,
                                                     uint64_t batch_id, WireSeqWs ws, uint32_t *__restrict__ out,
                                                     uint32_t *__restrict__ wait_client,
                                                     uint64_t *__restrict__ wait_startts,
                                                     uint32_t *__restrict__ wait_acks) {
    seq_emit<false>(cfg, buf, off, first, nb, batch_id, ws, out, wait_client, wait_startts, wait_acks);
}
__global__ __launch_bounds__(kBlock) void k_seq_emit_bytes(dv_wire_cfg cfg, const uint8_t *__restrict__ buf,
                                                           const uint64_t *__restrict__ off, uint32_t first,
                                                           uint32_t nb, uint64_t batch_id, WireSeqWs ws,
                                                           uint32_t *__restrict__ out,
                                                           uint32_t *__restrict__ wait_client,
                                                           uint64_t *__restrict__ wait_startts,
                                                           uint32_t *__restrict__ wait_acks) {
    seq_emit<true>(cfg, buf, off, first, nb, batch_id, ws, out, wait_client, wait_startts, wait_acks);
}

void launch_seq_plan(hipStream_t s, const dv_wire_cfg &cfg, const dv_wire_seq_in &in, const dv_wire_seq_out &out,
                     uint32_t nb, const WireSeqWs &ws) {
    const uint32_t nc = (nb + kWireChunk - 1) / kWireChunk, nodes = cfg.node_cnt, nbn = nb ? nb : 1;
    const uint32_t ntile = wire_seq_tiles(nbn, in.max_txn), grid = (nb + kWireWave - 1) / kWireWave;
    (void)hipMemsetAsync(ws.first, 0xFF, 2 * sizeof(uint32_t), s);  // kNoBatch
    if (nb) {
        if (cfg.workload == DV_TPCC)
            DV_LAUNCH(k_seq_check_tpcc, grid, kBlock, 0, s, without_tpcc(cfg), *cfg.tpcc, in.n_dest, in.buf, in.buf_len,
                      in.off, in.first_batch, nb, ws);
        else
            DV_LAUNCH(k_seq_check, grid, kBlock, 0, s, cfg, in.n_dest, in.buf, in.buf_len, in.off, in.first_batch, nb,
                      ws);
        DV_LAUNCH(k_wire_scan, nc, kBlock, 0, s, ws, nb);
    }
    DV_LAUNCH(k_seq_plan, 1, kBlock, 0, s, ws, in.first_batch, nb, in.n_batches, nc, in.max_txn);
    DV_LAUNCH(k_seq_dscan, nodes, kBlock, 0, s, ws, nbn);
    if (nb) DV_LAUNCH(k_seq_list, grid, kBlock, 0, s, ws, nbn, nodes);
    DV_LAUNCH(k_seq_tiles, dim3(ntile, nodes), kBlock, 0, s, ws, nodes);
    DV_LAUNCH(k_seq_chain, nodes, 64, 0, s, ws, nodes, ntile);
    DV_LAUNCH(k_seq_plan2, 1, 64, 0, s, ws, nodes, in.first_batch, out.cap, out.max_batches);
}

void launch_seq_emit(hipStream_t s, const dv_wire_cfg &cfg, const dv_wire_seq_in &in, const dv_wire_seq_out &out,
                     uint32_t nb, const WireSeqWs &ws) {
    const uint32_t nodes = cfg.node_cnt, nbn = nb ? nb : 1, ntile = wire_seq_tiles(nbn, in.max_txn);
    uint32_t *out32 = reinterpret_cast<uint32_t *>(out.out);
    const uint32_t grid = (nb + kWireWave - 1) / kWireWave;
    if (cfg.workload == DV_TPCC) {  // sizes 3 mod 4: entries at any byte
        DV_LAUNCH(k_seq_marks_bytes, dim3(ntile, nodes), kBlock, 0, s, ws, nodes, ntile, cfg.node_id, in.batch_id, out32,
                  out.batch_off, out.dest_first);
        if (nb)
            DV_LAUNCH(k_seq_emit_bytes, grid, kBlock, 0, s, without_tpcc(cfg), in.buf, in.off, in.first_batch, nbn,
                      in.batch_id, ws, out32, out.wait_client, out.wait_startts, out.wait_acks);
        return;
    }
    DV_LAUNCH(k_seq_marks, dim3(ntile, nodes), kBlock, 0, s, ws, nodes, ntile, cfg.node_id, in.batch_id, out32,
              out.batch_off, out.dest_first);
    if (nb)
        DV_LAUNCH(k_seq_emit, grid, kBlock, 0, s, cfg, in.buf, in.off, in.first_batch, nbn, in.batch_id, ws,
                  out32, out.wait_client, out.wait_startts, out.wait_acks);
}

// ---- the sequencer's acks in (dv_wire_sequence_acks_device): what
// dv_wire_sequence_acks (csrc/wire.cpp) does.  A wave per ack mbuf, staged as
// the ingests stage theirs, three times over the same bytes: the form, the
// per-txn ack counts and last positions (k_ack_count: vector atomics on scratch
// words, never on the wait list), the checks against the wait list and the
// completing acks per mbuf (k_ack_mark<false>), and, behind a scan, the
// completed txns in completing position order (k_ack_mark<true>).  That list
// goes through the reply packer as it is -- its count, scan, plan and emit over
// a third reply dialect, RspSeq -- and the wait list changes only behind the
// plan (k_ack_apply), where the whole call is known to stand.
namespace {
constexpr uint32_t kAckBytes = 88, kAckPer = (DV_WIRE_MSG_MAX - DV_WIRE_HDR) / kAckBytes;
static_assert(kAckPer == 46 && kAckPer <= 64, "a lane per ack");

// the wave's ack mbuf: bad where its form is wrong; lane m < count: message m,
// `mine` where it is an ack of batch_id for txn k of this sequencer
__device__ __forceinline__ bool ack_mbuf(const WaveBatch &w, const dv_wire_cfg &cfg, uint64_t batch_id, uint32_t n_txn,
                                         uint32_t &count, bool &mine, uint32_t &k) {
    const Stage &st = w.st;
    mine = false;
    count = k = 0;
    if (!w.live || w.bad) return true;
    count = st.u32(8);
    if (st.u32(0) != cfg.node_id || st.u32(4) >= cfg.node_cnt || count < 1 || count > kAckPer ||
        w.len != DV_WIRE_HDR + kAckBytes * count)
        return true;
    bool wrong = false;
    if (w.lane < count) {
        const uint32_t o = DV_WIRE_HDR + kAckBytes * w.lane;
        const uint64_t tid = st.u64(o + kCalTxnId), bid = st.u64(o + kCalBatchId);
        wrong = st.u32(o) != DV_WIRE_CALVIN_ACK || bid == kNoBatchId;
        if (!wrong && bid == batch_id) {
            wrong = tid % cfg.node_cnt != cfg.node_id || tid / cfg.node_cnt >= n_txn;
            mine = !wrong;
            k = (uint32_t)(tid / cfg.node_cnt);
        }
    }
    return __any(wrong);
}
}  // namespace

__global__ __launch_bounds__(kBlock) void k_ack_count(dv_wire_cfg cfg, const uint8_t *__restrict__ buf, uint64_t buf_len,
                                                      const uint64_t *__restrict__ off, uint32_t nb, uint64_t batch_id,
                                                      uint32_t n_txn, AckWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    const WaveBatch w = stage_wave_batch(s_img, buf, buf_len, off, 0, nb);
    uint32_t count, k;
    bool mine;
    const bool bad = ack_mbuf(w, cfg, batch_id, n_txn, count, mine, k);
    if (!w.live) return;
    if (bad) {
        if (w.lane == 0) {
            atomicMin(ws.first, w.b);
            atomicOr(ws.r.err, 1u);
        }
        return;
    }
    if (mine) {
        atomicAdd(&ws.acnt[k], 1u);
        atomicMax(&ws.alast[k], w.b * 64u + w.lane);  // the stream position: mbuf-major, message-minor
    }
    const uint32_t n_mine = (uint32_t)__popcll(__ballot(mine));
    if (w.lane == 0) {
        atomicAdd(&ws.counts[0], n_mine);
        atomicAdd(&ws.counts[1], count - n_mine);
    }
}

// LIST false: the txns' counts against the wait list, the completing acks per
// mbuf; true (behind the scan): the completed txns in position order
template <bool LIST>
__global__ __launch_bounds__(kBlock) void k_ack_mark(dv_wire_cfg cfg, const uint8_t *__restrict__ buf, uint64_t buf_len,
                                                     const uint64_t *__restrict__ off, uint32_t nb, uint64_t batch_id,
                                                     uint32_t n_txn, uint32_t n_dest,
                                                     const uint32_t *__restrict__ wait_client,
                                                     const uint32_t *__restrict__ wait_acks, AckWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    if (*ws.r.err) return;  // (a malformed mbuf, or LIST: any refusal -- the call fails whole)
    const WaveBatch w = stage_wave_batch(s_img, buf, buf_len, off, 0, nb);
    uint32_t count, k;
    bool mine;
    (void)ack_mbuf(w, cfg, batch_id, n_txn, count, mine, k);
    if (!w.live) return;
    bool completing = false;
    if (mine) {
        const uint32_t c = ws.acnt[k], wa = wait_acks[k];
        completing = c == wa && ws.alast[k] == w.b * 64u + w.lane;
        if (!LIST && (c > wa || (completing && wait_client[k] >= n_dest))) atomicOr(ws.err2, 1u);
    }
    const uint64_t bal = __ballot(completing);
    if (!LIST) {
        if (w.lane == 0) ws.bt[w.b] = (uint32_t)__popcll(bal);
    } else if (completing) {
        ws.done[ws.bt[w.b] + mask_rank(bal)] = k;
    }
}

// one workgroup: the completing acks in front of every mbuf, the completed txns
__global__ __launch_bounds__(kBlock) void k_ack_scan(AckWs ws, uint32_t nb) {
    __shared__ uint32_t lds4[4];
    const bool bad = *ws.r.err || *ws.err2;
    const uint32_t tot = bad ? 0u : block_chunk_scan256(ws.bt, nb, lds4);
    if (threadIdx.x != 0) return;
    ws.counts[2] = tot;
    if (bad) *ws.r.err = 1u;  // (the packer's plan refuses the call: nothing is written)
}

// behind the packer's plan: the call's record
__global__ __launch_bounds__(64) void k_ack_final(AckWs ws) {
    if (threadIdx.x != 0) return;
    const dv_wire_rsp_result p = *ws.r.res;
    dv_wire_seq_ack_result r{DV_ERR_ARG, *ws.first, 0, 0, 0, 0, 0};
    if (!*ws.r.err) {  // (else: malformed, over-acked or a client out of range: no count is reported)
        r.status = p.status;
        r.n_acks = ws.counts[0];
        r.n_skipped = ws.counts[1];
        r.n_done = ws.counts[2];
        r.n_batches = p.n_batches;
        r.n_bytes = p.n_bytes;
    }
    *ws.ares = r;
}

__global__ __launch_bounds__(kBlock) void k_ack_apply(AckWs ws, uint32_t n_txn, uint32_t *__restrict__ wait_acks) {
    if (ws.r.res->status != DV_OK) return;
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < n_txn) wait_acks[k] -= ws.acnt[k];
}

__global__ __launch_bounds__(kBlock) void k_rsp_emit_seq(RspSel sel, uint32_t nt, uint32_t node_id, uint32_t node_cnt,
                                                         const uint64_t *__restrict__ cst, ReplyWs ws,
                                                         uint32_t *__restrict__ out, uint64_t *__restrict__ batch_off) {
    rsp_emit<RspSeq>(sel, nt, node_id, node_cnt, nullptr, cst, ws, out, batch_off);
}

static RspSel ack_sel(const dv_wire_seq_ack_in &in, const AckWs &ws, uint32_t n_cap) {
    return RspSel{n_cap, in.n_txn, nullptr, ws.done, in.wait_client, ws.counts + 2};
}

void launch_ack_plan(hipStream_t s, const dv_wire_cfg &cfg, const dv_wire_seq_ack_in &in, const dv_wire_rsp_out &out,
                     uint32_t n_cap, const AckWs &ws) {
    const uint32_t nb = in.n_batches, grid = (nb + kWireWave - 1) / kWireWave, nt = reply_tiles(n_cap);
    (void)hipMemsetAsync(ws.first, 0xFF, sizeof(uint32_t), s);  // DV_WIRE_NO_BATCH
    (void)hipMemsetAsync(ws.zeroed, 0, ws.zeroed_bytes, s);     // err2, counts, acnt, alast
    (void)hipMemsetAsync(ws.r.err, 0, sizeof(uint32_t), s);
    if (nb) {
        DV_LAUNCH(k_ack_count, grid, kBlock, 0, s, cfg, in.buf, in.buf_len, in.off, nb, in.batch_id, in.n_txn, ws);
        DV_LAUNCH(k_ack_mark<false>, grid, kBlock, 0, s, cfg, in.buf, in.buf_len, in.off, nb, in.batch_id, in.n_txn,
                  in.n_dest, in.wait_client, in.wait_acks, ws);
    }
    DV_LAUNCH(k_ack_scan, 1, kBlock, 0, s, ws, nb);
    if (nb)
        DV_LAUNCH(k_ack_mark<true>, grid, kBlock, 0, s, cfg, in.buf, in.buf_len, in.off, nb, in.batch_id, in.n_txn,
                  in.n_dest, in.wait_client, in.wait_acks, ws);
    if (nt) {
        DV_LAUNCH(k_rsp_count, nt, kBlock, 0, s, ack_sel(in, ws, n_cap), in.n_dest, nt, ws.r);
        DV_LAUNCH(k_rsp_scan, in.n_dest, kBlock, 0, s, ws.r, nt);
    }
    DV_LAUNCH(k_rsp_plan, 1, kBlock, 0, s, ws.r, nt, in.n_dest, rsp_per<RspSeq>(), 4 * RspSeq::kDw, out.cap,
              out.max_batches, out.batch_off);
    DV_LAUNCH(k_ack_final, 1, 64, 0, s, ws);
}

void launch_ack_emit(hipStream_t s, const dv_wire_cfg &cfg, const dv_wire_seq_ack_in &in, const dv_wire_rsp_out &out,
                     uint32_t n_cap, const AckWs &ws) {
    const uint32_t nt = reply_tiles(n_cap);
    if (nt)
        DV_LAUNCH(k_rsp_emit_seq, nt, kBlock, 0, s, ack_sel(in, ws, n_cap), nt, cfg.node_id, cfg.node_cnt, in.wait_startts,
                  ws.r, reinterpret_cast<uint32_t *>(out.out), out.batch_off);
    if (in.n_txn) DV_LAUNCH(k_ack_apply, (in.n_txn + kBlock - 1) / kBlock, kBlock, 0, s, ws, in.n_txn, in.wait_acks);
}

}  // namespace dvcc
