// dvcc_wire.hip -- Deneva client batches decoded on the device.
//
// What csrc/wire.cpp does message by message on one core (dv_wire_open's
// checks, dv_wire_decode's arrays) for a receive queue's bytes already in
// device memory: YCSB CL_QRY batches, not CALVIN, taken at whole-batch
// granularity into a device-resident epoch (include/dvcc.h,
// dv_wire_ingest_device).  A batch is at most 4,096 bytes and a short chain of
// variable-length messages, so a wave takes one: its bytes staged in LDS,
// the chain walked once (at most 40 links), then every partition and request
// checked or scattered by all lanes.
//   k_wire_check   per batch {txns, accesses, longest txn}, the message
//                  offsets, and the first malformed batch
//   k_wire_scan    per chunk of kWireChunk batches: prefixes inside the chunk
//   k_wire_plan    one workgroup: the chunks' prefixes, the first batch that
//                  does not fit, the result record, the closing boundary
//   k_wire_emit    the taken batches' boundaries, reply fields and accesses
// and, for the replies, the committed txns' fields compacted in txn order
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
constexpr uint32_t kMsgHdr = 76;       // rtype, txn_id, mq_time, 7 latencies (Message::mget_size, not CALVIN)
constexpr uint32_t kMsgFixed = 92;     // ... client_startts, the partition count
constexpr uint32_t kReqBytes = 24;     // sizeof(ycsb_request)
constexpr uint32_t kReqMax = 128;      // the engine's longest txn (kMaxPos)
constexpr uint32_t kNoBatch = 0xFFFFFFFFu;

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

}  // namespace

// Whatever dv_wire_open refuses makes the batch bad, whole.  Every length is
// compared as the 64-bit count it is before it is multiplied: a count of
// 2^61 + 1 fails `n > lim`, it never reaches n * 24.
__global__ __launch_bounds__(kBlock) void k_wire_check(dv_wire_cfg cfg, const uint8_t *__restrict__ buf,
                                                       uint64_t buf_len, const uint64_t *__restrict__ off,
                                                       uint32_t first, uint32_t nb, WireWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint32_t s_rq[kWireWave][64], s_pp[kWireWave][64];  // requests / partitions before message m
    __shared__ uint16_t s_mo[kWireWave][64], s_p2[kWireWave][64];  // message m's offset, its request count's
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * kWireWave + wave;
    const bool live = b < nb;
    uint64_t o0 = 0;
    uint32_t len = 0;
    bool bad = live && !batch_span(off, first + b, buf_len, o0, len);
    const bool parse = live && !bad;
    Stage st{reinterpret_cast<const uint32_t *>(s_img[wave]), 0};
    if (parse) st.sh = stage_batch(buf + o0, len, s_img[wave], lane);
    __syncthreads();
    uint32_t count = 0, my_off = 0, my_np = 0, my_n = 0, my_p2 = 0;
    if (parse) {
        // create_messages' asserts (message.cpp:39-41), then the chain: every lane walks it
        count = st.u32(8);
        bad = st.u32(0) != cfg.node_id || st.u32(4) == cfg.node_id || count == 0 || count > kWireMaxMsg;
        const uint32_t lim = cfg.max_req && cfg.max_req < kReqMax ? cfg.max_req : kReqMax;
        uint32_t pos = DV_WIRE_HDR;
        for (uint32_t m = 0; !bad && m < count; m++) {
            if (pos + kMsgFixed > len) { bad = true; break; }
            const uint64_t np = st.u64(pos + kMsgHdr + 8);
            if (st.u32(pos) != DV_WIRE_CL_QRY || np > DV_TPCC_MAX_PARTS) { bad = true; break; }
            const uint32_t p2 = pos + kMsgFixed + (uint32_t)np * 8u;
            if (p2 + 8 > len) { bad = true; break; }
            const uint64_t n = st.u64(p2);
            if (n > lim) { bad = true; break; }
            const uint32_t end = p2 + 8 + (uint32_t)n * kReqBytes;
            if (end > len) { bad = true; break; }
            if (lane == m) {
                my_off = pos;
                my_np = (uint32_t)np;
                my_n = (uint32_t)n;
                my_p2 = p2;
            }
            pos = end;
        }
        if (!bad && pos != len) bad = true;  // exactly `count` messages fill exactly `len` bytes
    }
    // (a bad batch's lanes hold zeros or a part of the chain: its tables are not read)
    const uint32_t rq_in = wave_incl_sum(my_n, lane), pp_in = wave_incl_sum(my_np, lane);
    const uint32_t tot_rq = __shfl(rq_in, 63, 64), tot_pp = __shfl(pp_in, 63, 64);
    uint32_t mx = my_n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t y = __shfl_xor(mx, o, 64);
        mx = y > mx ? y : mx;
    }
    s_rq[wave][lane] = rq_in - my_n;
    s_pp[wave][lane] = pp_in - my_np;
    s_mo[wave][lane] = (uint16_t)my_off;
    s_p2[wave][lane] = (uint16_t)my_p2;
    __syncthreads();
    bool wrong = false;
    if (parse && !bad) {
        for (uint32_t q = lane; q < tot_pp; q += 64) {  // every partition named below part_cnt
            const uint32_t m = last_le64(s_pp[wave], q);
            wrong |= st.u64(s_mo[wave][m] + kMsgFixed + (q - s_pp[wave][m]) * 8u) >= cfg.part_cnt;
        }
        for (uint32_t r = lane; r < tot_rq; r += 64) {  // RD / WR of keys inside the table
            const uint32_t m = last_le64(s_rq[wave], r);
            const uint32_t ro = s_p2[wave][m] + 8u + (r - s_rq[wave][m]) * kReqBytes;
            wrong |= st.u32(ro) > DV_WR || st.u64(ro + 8) >= cfg.synth_table_size;
        }
    }
    bad = bad || __any(wrong);
    if (!live) return;
    if (!bad && lane < count) ws.moff[(uint64_t)b * kWireMaxMsg + lane] = (uint16_t)my_off;
    if (lane == 0) {
        ws.bt[b] = bad ? 0u : count;
        ws.ba[b] = bad ? 0u : tot_rq;
        ws.bm[b] = bad ? (uint8_t)0 : (uint8_t)mx;
        if (bad) atomicMin(ws.first_bad, b);
    }
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
// malformed batch (k_wire_check's first_bad), or the first whose txns or
// accesses, added to those before it, pass the capacities -- the running
// sums only grow, so that is the first batch of the first chunk that does not
// fit whole.  (A bad batch counts nothing: it never is the capacity cut.)
__global__ __launch_bounds__(kBlock) void k_wire_plan(WireWs ws, uint32_t first, uint32_t nb, uint32_t n_batches,
                                                      uint32_t nc, dv_wire_dev_out out, uint64_t next_txn) {
    __shared__ uint32_t lds4[4], s_chunk, s_cut, s_max;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_chunk = nc;
        s_cut = nb;
        s_max = 0;
    }
    const uint32_t tot_t = block_chunk_scan256(ws.ct, nc, lds4);
    const uint32_t tot_a = block_chunk_scan256(ws.ca, nc, lds4);
    __syncthreads();
    for (uint32_t i = tid; i < nc; i += kBlock) {
        const uint32_t it = i + 1 < nc ? ws.ct[i + 1] : tot_t, ia = i + 1 < nc ? ws.ca[i + 1] : tot_a;
        if (it > out.max_txn || ia > out.max_acc) atomicMin(&s_chunk, i);
    }
    __syncthreads();
    const uint32_t cc = s_chunk;
    if (cc < nc) {
        const uint32_t base = cc * kWireChunk;
        const uint32_t n = nb - base < kWireChunk ? nb - base : kWireChunk;
        const uint32_t t0 = ws.ct[cc], a0 = ws.ca[cc];
        const uint32_t ch_t = (cc + 1 < nc ? ws.ct[cc + 1] : tot_t) - t0, ch_a = (cc + 1 < nc ? ws.ca[cc + 1] : tot_a) - a0;
        for (uint32_t j = tid; j < n; j += kBlock) {
            const uint32_t it = t0 + (j + 1 < n ? ws.bt[base + j + 1] : ch_t);
            const uint32_t ia = a0 + (j + 1 < n ? ws.ba[base + j + 1] : ch_a);
            if (it > out.max_txn || ia > out.max_acc) atomicMin(&s_cut, base + j);
        }
    }
    __syncthreads();
    const uint32_t cut = s_cut, fb = *ws.first_bad;
    const uint32_t k = fb < cut ? fb : cut;  // batches taken (<= nb)
    const uint32_t full = k / kWireChunk;
    uint32_t mx = 0;
    for (uint32_t i = tid; i < full; i += kBlock) mx = ws.cm[i] > mx ? ws.cm[i] : mx;
    for (uint32_t j = full * kWireChunk + tid; j < k; j += kBlock) mx = ws.bm[j] > mx ? ws.bm[j] : mx;
    atomicMax(&s_max, mx);
    __syncthreads();
    if (tid != 0) return;
    const uint32_t n_txn = k == nb ? tot_t : ws.ct[full] + ws.bt[k];
    const uint32_t n_acc = k == nb ? tot_a : ws.ca[full] + ws.ba[k];
    int32_t status = DV_OK;
    if (fb < nb && fb <= cut) status = DV_ERR_ARG;                // the malformed batch comes first
    else if (cut < nb) status = cut ? DV_WIRE_MORE : DV_ERR_ARG;  // (the first batch: it would never fit)
    else if (first + nb < n_batches) status = DV_WIRE_MORE;       // (the call's window of max_txn + 1 batches)
    dv_wire_dev_result r;
    r.status = status;
    r.n_taken = first + k;
    r.n_txn = n_txn;
    r.max_txn_acc = s_max;
    r.n_acc = n_acc;
    r.next_txn = next_txn + n_txn;
    *ws.res = r;
    out.txn_begin[n_txn] = n_acc;  // (n_txn <= max_txn)
    *out.n_acc_dev = n_acc;
}

// the taken batches (below the plan's n_taken), a wave each: lane m message
// m's boundary and reply fields, then all lanes the batch's requests in
// order -- consecutive lanes, consecutive accesses
__global__ __launch_bounds__(kBlock) void k_wire_emit(dv_wire_cfg cfg, const uint8_t *__restrict__ buf,
                                                      const uint64_t *__restrict__ off, uint32_t first,
                                                      dv_wire_dev_out out, uint64_t next_txn, WireWs ws) {
    __shared__ uint4 s_img[kWireWave][kStageQ];
    __shared__ uint32_t s_rq[kWireWave][64];
    __shared__ uint16_t s_p2[kWireWave][64];
    const uint32_t taken = ws.res->n_taken - first;
    if (blockIdx.x * kWireWave >= taken) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * kWireWave + wave;
    const bool live = b < taken;  // (checked by k_wire_check: its span and every field are good)
    Stage st{reinterpret_cast<const uint32_t *>(s_img[wave]), 0};
    if (live) {
        const uint64_t o0 = off[first + b];
        st.sh = stage_batch(buf + o0, (uint32_t)(off[first + b + 1] - o0), s_img[wave], lane);
    }
    __syncthreads();
    uint32_t count = 0, src = 0, my_n = 0, my_p2 = 0, t0 = 0, a0 = 0;
    uint64_t cst = 0;
    if (live) {
        src = st.u32(4);
        count = st.u32(8);
        t0 = ws.ct[b / kWireChunk] + ws.bt[b];
        a0 = ws.ca[b / kWireChunk] + ws.ba[b];
        if (lane < count) {
            const uint32_t mo = ws.moff[(uint64_t)b * kWireMaxMsg + lane];
            cst = st.u64(mo + kMsgHdr);
            my_p2 = mo + kMsgFixed + st.u32(mo + kMsgHdr + 8) * 8u;
            my_n = st.u32(my_p2);
        }
    }
    const uint32_t rq_in = wave_incl_sum(my_n, lane);
    const uint32_t tot_rq = __shfl(rq_in, 63, 64);
    s_rq[wave][lane] = rq_in - my_n;
    s_p2[wave][lane] = (uint16_t)my_p2;
    __syncthreads();
    if (!live) return;
    if (lane < count) {
        const uint32_t t = t0 + lane;
        out.txn_begin[t] = a0 + rq_in - my_n;
        // WorkerThread::get_next_txn_id for one worker (worker_thread.cpp:453-458)
        if (out.txn_id) out.txn_id[t] = cfg.node_id + (uint64_t)cfg.node_cnt * (next_txn + t);
        if (out.client_startts) out.client_startts[t] = cst;
        if (out.return_node) out.return_node[t] = src;
    }
    for (uint32_t r = lane; r < tot_rq; r += 64) {
        const uint32_t m = last_le64(s_rq[wave], r);
        const uint32_t ro = s_p2[wave][m] + 8u + (r - s_rq[wave][m]) * kReqBytes;
        const uint32_t acctype = st.u32(ro);
        const uint64_t key = st.u64(ro + 8);
        const uint32_t a = a0 + r;
        if (out.recs32) out.recs32[a] = (uint32_t)key | (acctype == DV_WR ? AR_WR : 0u);
        if (out.keys) {
            out.keys[a] = key;
            out.types[a] = (uint8_t)acctype;
            out.acc_txn[a] = t0 + m;
        }
        if (out.owner) out.owner[a] = (uint8_t)(key % cfg.part_cnt);  // key_to_part
    }
}

uint64_t wire_ws_bytes(uint32_t nb) {
    const uint64_t n = nb ? nb : 1, nc = (n + kWireChunk - 1) / kWireChunk;
    // (every array's size a multiple of 8 bytes: moff first, the words, the bytes last)
    return n * kWireMaxMsg * 2 + 2 * ((n + 1) & ~1ull) * 4 + 3 * ((nc + 1) & ~1ull) * 4 + 8 +
           sizeof(dv_wire_dev_result) + ((n + 7) & ~7ull);
}

WireWs wire_ws_carve(void *base, uint32_t nb) {
    const uint64_t n = nb ? nb : 1, nc = (n + kWireChunk - 1) / kWireChunk;
    const uint64_t n2 = (n + 1) & ~1ull, nc2 = (nc + 1) & ~1ull;
    WireWs w;
    char *p = static_cast<char *>(base);
    w.res = reinterpret_cast<dv_wire_dev_result *>(p);
    p += sizeof(dv_wire_dev_result);
    w.first_bad = reinterpret_cast<uint32_t *>(p);
    p += 8;
    w.moff = reinterpret_cast<uint16_t *>(p);
    p += n * kWireMaxMsg * 2;
    w.bt = reinterpret_cast<uint32_t *>(p);
    p += n2 * 4;
    w.ba = reinterpret_cast<uint32_t *>(p);
    p += n2 * 4;
    w.ct = reinterpret_cast<uint32_t *>(p);
    p += nc2 * 4;
    w.ca = reinterpret_cast<uint32_t *>(p);
    p += nc2 * 4;
    w.cm = reinterpret_cast<uint32_t *>(p);
    p += nc2 * 4;
    w.bm = reinterpret_cast<uint8_t *>(p);
    return w;
}

void launch_wire_plan(hipStream_t s, const dv_wire_cfg &cfg, const uint8_t *buf, uint64_t buf_len,
                      const uint64_t *off, uint32_t first, uint32_t nb, uint32_t n_batches,
                      const dv_wire_dev_out &out, uint64_t next_txn, const WireWs &ws) {
    const uint32_t nc = (nb + kWireChunk - 1) / kWireChunk;
    (void)hipMemsetAsync(ws.first_bad, 0xFF, sizeof(uint32_t), s);  // kNoBatch
    static_assert(kNoBatch == 0xFFFFFFFFu, "the memset's value");
    if (nb) {
        DV_LAUNCH(k_wire_check, (nb + kWireWave - 1) / kWireWave, kBlock, 0, s, cfg, buf, buf_len, off, first, nb, ws);
        DV_LAUNCH(k_wire_scan, nc, kBlock, 0, s, ws, nb);
    }
    DV_LAUNCH(k_wire_plan, 1, kBlock, 0, s, ws, first, nb, n_batches, nc, out, next_txn);
}

void launch_wire_emit(hipStream_t s, const dv_wire_cfg &cfg, const uint8_t *buf, const uint64_t *off,
                      uint32_t first, uint32_t nb, const dv_wire_dev_out &out, uint64_t next_txn,
                      const WireWs &ws) {
    if (!nb) return;
    DV_LAUNCH(k_wire_emit, (nb + kWireWave - 1) / kWireWave, kBlock, 0, s, cfg, buf, off, first, out, next_txn, ws);
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

}  // namespace dvcc
